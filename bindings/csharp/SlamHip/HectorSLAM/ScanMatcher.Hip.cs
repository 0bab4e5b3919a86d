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

        /// <summary>... with the match report (slamhip_hs_match_report), produced in the same launch; the pose is the plain call's.</summary>
        public Vector3 MatchData(MapRepMultiMap multiMap, ScanCloud scan, Vector3 hintPose, out MatchReport report)
        {
            Native.Check(Native.slamhip_hs_set_match_threads(multiMap.Pyramid.Ptr, matchThreads));
            multiMap.SetScan(scan);
            Native.Check(Native.slamhip_hs_match_report(multiMap.Pyramid.Ptr, hintPose, out Vector3 pose, out report));
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

        /// <summary>... with the match report on that grid's level (slamhip_hs_match_level_report).</summary>
        public unsafe Vector3 MatchData(OccGridMap gridMap, ScanCloud scan, Vector3 hintPose, out MatchReport report)
        {
            Native.Check(Native.slamhip_hs_set_match_threads(gridMap.Pyramid.Ptr, matchThreads));
            fixed (Vector2* p = System.Runtime.InteropServices.CollectionsMarshal.AsSpan(scan.Points))
                Native.Check(Native.slamhip_hs_set_scan(gridMap.Pyramid.Ptr, p, scan.Points.Count, new Vector2(scan.Pose.X, scan.Pose.Y)));
            Native.Check(Native.slamhip_hs_match_level_report(gridMap.Pyramid.Ptr, gridMap.Level, hintPose, gridMap.EstimateIterations, out Vector3 pose, out report));
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

        /// <summary>... with every match's report (slamhip_hs_match_batch_report).</summary>
        public unsafe Vector3[] MatchDataBatch(MapRepMultiMap multiMap, ScanCloud scan, Vector3[] hintPoses, out MatchReport[] reports)
        {
            Native.Check(Native.slamhip_hs_set_match_threads(multiMap.Pyramid.Ptr, matchThreads));
            multiMap.SetScan(scan);
            Vector3[] poses = new Vector3[hintPoses.Length];
            reports = new MatchReport[hintPoses.Length];
            fixed (Vector3* h = hintPoses)
            fixed (Vector3* o = poses)
            fixed (MatchReport* r = reports)
                Native.Check(Native.slamhip_hs_match_batch_report(multiMap.Pyramid.Ptr, h, hintPoses.Length, o, r));
            return poses;
        }

        /// <summary>The best of many hints, picked on the device by the smallest residual, ties to the lowest index
        /// (slamhip_hs_match_best): only the winner comes back.  Whether its residual is good enough is the caller's decision.</summary>
        public unsafe Vector3 MatchDataBest(MapRepMultiMap multiMap, ScanCloud scan, Vector3[] hintPoses, out int index, out MatchReport report)
        {
            Native.Check(Native.slamhip_hs_set_match_threads(multiMap.Pyramid.Ptr, matchThreads));
            multiMap.SetScan(scan);
            Vector3 pose;
            fixed (Vector3* h = hintPoses)
                Native.Check(Native.slamhip_hs_match_best(multiMap.Pyramid.Ptr, h, hintPoses.Length, out pose, out index, out report));
            return pose;
        }

        /// <summary>Lattice search, then the best nodes of the maxHints highest-scoring headings refined by MatchDataBest
        /// (slamhip_hs_relocalise): the winner with its report and where it started from.  Poses in the window's frame.</summary>
        public unsafe Vector3 Relocalise(MapRepMultiMap multiMap, ScanCloud scan, LatticeSpec lattice, int maxHints, out MatchReport report, out RelocInfo info)
        {
            Native.Check(Native.slamhip_hs_set_match_threads(multiMap.Pyramid.Ptr, matchThreads));
            multiMap.SetScan(scan);
            Native.Check(Native.slamhip_hs_relocalise(multiMap.Pyramid.Ptr, lattice, maxHints, out Vector3 pose, out report, out info));
            return pose;
        }

        /// <summary>Relocalise anywhere in the world behind the window (slamhip_hs_relocalise_world; backing must be on): the world
        /// lattice search, the window shifted to the best node, the best nodes that lie in the new window refined by MatchDataBest.
        /// The pose is in the NEW window's frame; info.Dx, info.Dy say how the window moved.</summary>
        public unsafe Vector3 RelocaliseWorld(MapRepMultiMap multiMap, ScanCloud scan, LatticeSpec lattice, int maxHints, out MatchReport report, out WorldRelocInfo info)
        {
            Native.Check(Native.slamhip_hs_set_match_threads(multiMap.Pyramid.Ptr, matchThreads));
            multiMap.SetScan(scan);
            Native.Check(Native.slamhip_hs_relocalise_world(multiMap.Pyramid.Ptr, lattice, maxHints, out Vector3 pose, out report, out info));
            multiMap.MarkStale();
            return pose;
        }

        /// <summary>The hint list of a relocalisation around centre = (x, y, theta): every combination of x, y in centre +- k * stepXy
        /// (k * stepXy &lt;= halfXy) and theta in centre +- j * stepTheta (j * stepTheta &lt;= halfTheta).  The centre itself comes first
        /// (ties in MatchDataBest go to the lowest index); the rest follow in x-major, then y, then theta order.  Pure host code.</summary>
        public static Vector3[] HintLattice(Vector3 centre, float halfXy, float stepXy, float halfTheta, float stepTheta)
        {
            if (!(stepXy > 0 && stepTheta > 0 && halfXy >= 0 && halfTheta >= 0))
                throw new ArgumentOutOfRangeException(nameof(stepXy), "steps must be positive and half-widths non-negative");
            int nxy = (int)Math.Floor((double)halfXy / stepXy + 1e-9), nth = (int)Math.Floor((double)halfTheta / stepTheta + 1e-9);
            var hints = new System.Collections.Generic.List<Vector3> { centre };
            for (int i = -nxy; i <= nxy; i++)
                for (int j = -nxy; j <= nxy; j++)
                    for (int k = -nth; k <= nth; k++)
                        if (i != 0 || j != 0 || k != 0)
                            hints.Add(new Vector3((float)(centre.X + (double)i * stepXy), (float)(centre.Y + (double)j * stepXy),
                                                  (float)(centre.Z + (double)k * stepTheta)));
            return hints.ToArray();
        }

        public void Dispose()
        {
            GC.SuppressFinalize(this);
        }
    }
}
