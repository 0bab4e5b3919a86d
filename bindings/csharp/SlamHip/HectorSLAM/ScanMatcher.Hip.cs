// HectorSLAM.Matcher.ScanMatcher on the GPU (reference: HectorSLAM/Matcher/ScanMatcher.cs:18-272): the Gauss-Newton
// alignment of a scan to the occupancy pyramid -- all levels and iterations of a match are ONE kernel launch (one
// workgroup: bilinear taps, Hessian sums, 3x3 solve, clamp, next iteration).  Nothing is threaded on the host.  By default
// numThreads is accepted for source compatibility, and poses agree with the reference to 1e-4 m / 1e-4 rad (its own result
// moves by that much with its thread count: binary32 chunk sums, :149-195).  With referenceSummation the device sums in the
// reference's order for numThreads (slamhip_hs_set_match_threads, set on the target pyramid before every match): H, dTr and
// the pose are then the reference's bits wherever both read the same cell probabilities.
using System;
using System.Numerics;
using BaseSLAM;
using HectorSLAM.Main;
using HectorSLAM.Map;
using Microsoft.Extensions.Logging;
using SlamHip;

namespace HectorSLAM.Matcher
{
    public class ScanMatcher : IDisposable
    {
        private readonly ILogger logger;
        private readonly int matchThreads;                               // what every match sets: 0 (the device's order) or numThreads

        public ScanMatcher(int numThreads, ILogger logger = null)
            : this(numThreads, logger, false)
        {
        }

        /// <param name="referenceSummation">sum as the reference does with numThreads threads (1..64), bit for bit</param>
        public ScanMatcher(int numThreads, ILogger logger, bool referenceSummation)
        {
            this.logger = logger;
            if (referenceSummation && (numThreads < 1 || numThreads > 64))
                throw new ArgumentOutOfRangeException(nameof(numThreads), "reference summation needs 1..64 threads");
            matchThreads = referenceSummation ? numThreads : 0;
        }

        /// <summary>Coarse-to-fine over every level of the pyramid (ScanMatcher.cs:41-54).</summary>
        public Vector3 MatchData(MapRepMultiMap multiMap, ScanCloud scan, Vector3 hintPose)
        {
            Native.Check(Native.slamhip_hs_set_match_threads(multiMap.Pyramid.Ptr, matchThreads));
            multiMap.SetScan(scan);
            Native.Check(Native.slamhip_hs_match(multiMap.Pyramid.Ptr, hintPose, out Vector3 pose));
            return pose;
        }

        /// <summary>One grid, gridMap.EstimateIterations iterations (ScanMatcher.cs:64-84).</summary>
        public unsafe Vector3 MatchData(OccGridMap gridMap, ScanCloud scan, Vector3 hintPose)
        {
            if (scan.Points.Count == 0) return hintPose;                 // :82-83
            Native.Check(Native.slamhip_hs_set_match_threads(gridMap.Pyramid.Ptr, matchThreads));
            fixed (Vector2* p = System.Runtime.InteropServices.CollectionsMarshal.AsSpan(scan.Points))
                Native.Check(Native.slamhip_hs_set_scan(gridMap.Pyramid.Ptr, p, scan.Points.Count, new Vector2(scan.Pose.X, scan.Pose.Y)));
            Native.Check(Native.slamhip_hs_match_level(gridMap.Pyramid.Ptr, gridMap.Level, hintPose, gridMap.EstimateIterations, out Vector3 pose));
            return pose;
        }

        /// <summary>Many hints against the same scan and maps in one launch (new: relocalisation, particle filters).</summary>
        public unsafe Vector3[] MatchDataBatch(MapRepMultiMap multiMap, ScanCloud scan, Vector3[] hintPoses)
        {
            Native.Check(Native.slamhip_hs_set_match_threads(multiMap.Pyramid.Ptr, matchThreads));
            multiMap.SetScan(scan);
            Vector3[] poses = new Vector3[hintPoses.Length];
            fixed (Vector3* h = hintPoses)
            fixed (Vector3* o = poses)
                Native.Check(Native.slamhip_hs_match_batch(multiMap.Pyramid.Ptr, h, hintPoses.Length, o));
            return poses;
        }

        public void Dispose()
        {
            GC.SuppressFinalize(this);
        }
    }
}
