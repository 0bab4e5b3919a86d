// SlamHip.Native.cs -- P/Invoke surface of libslamhip.so (include/slamhip.h), one declaration per C entry point the
// managed shims use.  Every function returns an int32 status (0 = OK); Check() turns anything else into an
// InvalidOperationException carrying slamhip_last_error().  Structs crossing the boundary are blittable:
// Vector2 / Vector3 / Vector4 (8 / 12 / 16 bytes), LogOddsCell {int UpdateIndex; float Value} (8 bytes), MatchReport
// (slamhip_match_report: 19 four-byte fields, 76 bytes) and SearchReport (slamhip_search_report: 9 doubles + 12 ints, 120 bytes).
//
// Source only: the build image of this repository has no .NET SDK; the same symbols are exercised by the ctypes
// binding (slam.net_amd/capi.py) and by the GPU tests.
using System;
using System.Numerics;
using System.Runtime.InteropServices;

namespace SlamHip
{
    /// <summary>slamhip_match_report (include/slamhip.h): the match evaluated once more at the pose it ends on -- H and dTr of
    /// GetCompleteHessianDerivs (ScanMatcher.cs:135-204) at PoseMap on the report level, the residual (sum over all scan points of
    /// (1 - M)^2, a point outside the map adding 1) and how many points fell inside the map.  19 four-byte fields, 76 bytes.
    /// The library sets no acceptance threshold: what residual means "lost" is the host's decision.</summary>
    /// <summary>slamhip_search_report: what a caller needs to judge a CoreSLAM Monte-Carlo search (CoreSLAMProcessor.cs:624-710) -- the
    /// distance of the un-jittered pose (Dist0), the runner-up and the tie count, the candidates without a point in the map, the
    /// winner's in-map count (:247) against NPoints, and over the band set (scored candidates within Band of the best distance) the
    /// sums of the jitters and of their products, from which the host forms mean and covariance.  9 doubles + 12 ints, 120 bytes.
    /// The library sets no threshold: what margin or spread means "lost" is the host's decision.</summary>
    [StructLayout(LayoutKind.Sequential, Pack = 8)]
    public struct SearchReport
    {
        public double SumDx, SumDy, SumDtheta;
        public double SumDxDx, SumDxDy, SumDxDtheta, SumDyDy, SumDyDtheta, SumDthetaDtheta;
        public int BestDist, BestIndex;
        public int RunnerDist, RunnerIndex;
        public int Dist0;
        public int NCandidates, NUnscored, NTies;
        public int Band, NBand;
        public int NInMap, NPoints;
    }

    [StructLayout(LayoutKind.Sequential, Pack = 4)]
    public struct MatchReport
    {
        public float PoseMapX, PoseMapY, PoseMapTheta;
        public float H11, H12, H13, H21, H22, H23, H31, H32, H33;
        public float DTrX, DTrY, DTrTheta;
        public float Residual;
        public int InMapCount;
        public int PointCount;
        public int Level;

        public Vector3 PoseMap => new Vector3(PoseMapX, PoseMapY, PoseMapTheta);
        public Vector3 DTr => new Vector3(DTrX, DTrY, DTrTheta);
        /// <summary>Residual per scan point: 0 a perfect fit, 0.25 unobserved cells, 1 off the map.</summary>
        public float ResidualPerPoint => PointCount > 0 ? Residual / PointCount : 0f;
    }

    /// <summary>slamhip_backing_stats (include/slamhip.h): the backing store of the scrolling window -- tiles in the directory, bytes of
    /// the device pool allocated so far, its capacity, and the cells evicted, restored and dropped since backing was switched on
    /// (host-side sums of job areas).  6 longs + 2 ints, 56 bytes; all zero while backing is off.</summary>
    [StructLayout(LayoutKind.Sequential, Pack = 8)]
    public struct BackingStats
    {
        public long Tiles, Bytes, CapacityBytes;
        public long EvictedCells, RestoredCells, DroppedCells;
        public int Tile, On;
    }

    /// <summary>slamhip_lattice_spec (include/slamhip.h): the pose lattice of the relocalisation search -- translations by whole cells
    /// of pyramid level Level, ix in [-Nx, Nx], iy in [-Ny, Ny], around (CentreX, CentreY), headings CentreTheta + k * DTheta,
    /// k = 0 .. NTheta - 1.  The centre is a pose in the window's frame (a world pose for HectorSLAMProcessor.Relocalise).
    /// 8 four-byte fields, 32 bytes.</summary>
    [StructLayout(LayoutKind.Sequential)]
    public struct LatticeSpec
    {
        public int Level;
        public int Nx, Ny;
        public int NTheta;
        public float CentreX, CentreY, CentreTheta;
        public float DTheta;
    }

    /// <summary>slamhip_reloc_info (include/slamhip.h): the hints a relocalisation handed to the matcher and the lattice node the
    /// winner started from.  7 ints, 28 bytes.</summary>
    [StructLayout(LayoutKind.Sequential)]
    public struct RelocInfo
    {
        public int HintCount, BestHint;
        public int K, Ix, Iy;
        public int Score, TopScore;
    }

    /// <summary>slamhip_world_reloc_info (include/slamhip.h): the fields of RelocInfo, then the shift the relocalisation applied
    /// (level-0 cells) and the hints dropped for lying outside the new window.  10 ints, 40 bytes.</summary>
    [StructLayout(LayoutKind.Sequential)]
    public struct WorldRelocInfo
    {
        public int HintCount, BestHint;
        public int K, Ix, Iy;
        public int Score, TopScore;
        public int Dx, Dy;
        public int FarCount;
    }

    /// <summary>slamhip_trace_beam (include/slamhip.h): what the map holds along one beam of a trace.  Da: -1 ignored, 0 the
    /// sensor's own cell, else the length of the walked line; First: the step of the first occupied cell, or -1; UnknownCount: the
    /// unknown cells in front of it; EndClass: the class of the end cell (1 occupied, 2 free, 0 neither); Hx, Hy: the cell of
    /// step First in window-frame cells of the level.  6 ints, 24 bytes.</summary>
    [StructLayout(LayoutKind.Sequential)]
    public struct TraceBeam
    {
        public int Da, First, UnknownCount, EndClass;
        public int Hx, Hy;
    }

    /// <summary>slamhip_trace_summary (include/slamhip.h): one pose's beams counted -- by status, those that reach an obstacle at
    /// their end cell, those blocked in front of it, those that end on a free cell -- and the unknown cells they cross.  6 ints and
    /// a long, 32 bytes.</summary>
    [StructLayout(LayoutKind.Sequential)]
    public struct TraceSummary
    {
        public int WalkedCount, SameCount, IgnoredCount;
        public int EndHitCount, BlockedCount, EndFreeCount;
        public long UnknownCells;
    }

    /// <summary>slamhip_distance_summary (include/slamhip.h): one pose's scan points against the distance field -- counted and
    /// ignored points, those whose end cell is a site (ZeroCount), those with no site within the radius (CappedCount), and the sum
    /// of the squared cell distances of the counted points.  4 ints and a long, 24 bytes.</summary>
    [StructLayout(LayoutKind.Sequential)]
    public struct DistanceSummary
    {
        public int CountedCount, IgnoredCount;
        public int ZeroCount, CappedCount;
        public long SumD2;
    }

    /// <summary>slamhip_pair_summary (include/slamhip.h): one pose's scan points against the nearest-site field -- counted, ignored
    /// and matched points (a site within the radius of the end cell), those whose end cell is a site (ZeroCount), and over the
    /// matched points the sum of the squared offsets and the sums of the end cells e, their sites q and the four products, in
    /// window-frame cells of the level: what one closed-form alignment step needs.  4 ints and 9 longs, 88 bytes.</summary>
    [StructLayout(LayoutKind.Sequential)]
    public struct PairSummary
    {
        public int CountedCount, IgnoredCount;
        public int MatchedCount, ZeroCount;
        public long SumD2;
        public long SumEx, SumEy, SumQx, SumQy;
        public long SumExQx, SumEyQy, SumExQy, SumEyQx;
    }

    /// <summary>slamhip_frontier_cluster (include/slamhip.h): one connected cluster of frontier cells -- free cells that touch the
    /// unknown -- of one level: its seed (first cell in row-major order), cells, runs, bounding box (inclusive) and the sums of its
    /// cells' coordinates (centroid = sum / cells).  8 ints and 2 longs, 48 bytes.</summary>
    [StructLayout(LayoutKind.Sequential)]
    public struct FrontierCluster
    {
        public int SeedX, SeedY;
        public int CellCount, RunCount;
        public int XMin, YMin, XMax, YMax;
        public long SumX, SumY;
    }

    /// <summary>slamhip_frontier_summary (include/slamhip.h): the class map's rectangle, the frontier cells, runs and clusters of the
    /// whole level, and the clusters kept (cells >= minCells) and returned.  10 ints, 40 bytes.</summary>
    [StructLayout(LayoutKind.Sequential)]
    public struct FrontierSummary
    {
        public int MapX0, MapY0, MapWidth, MapHeight;
        public int FrontierCellCount, RunCount, ClusterCount;
        public int KeptCount, ReturnedCount;
        public int KeptCells;
    }

    /// <summary>slamhip_nav_spec (include/slamhip.h): the level, window (0) or world (1), the sites the clearance is kept from (2
    /// obstacles, 3 obstacles or the unknown), the clearance in cells (0 .. 254) and the cost cap (0: none).  5 words, 20 bytes.</summary>
    [StructLayout(LayoutKind.Sequential)]
    public struct NavSpec
    {
        public int Level, World, SiteMask, Clearance;
        public uint MaxCost;
    }

    /// <summary>slamhip_nav_goal_result (include/slamhip.h): the least cost-to-go over a goal rectangle (Unreached: no reached cell),
    /// the cell that has it and the reached cells of the rectangle.  16 bytes.</summary>
    [StructLayout(LayoutKind.Sequential)]
    public struct NavGoalResult
    {
        public const uint Unreached = 0xFFFFFFFFu;
        public uint Cost;
        public int BestX, BestY;
        public int ReachedCount;
    }

    /// <summary>slamhip_nav_path (include/slamhip.h): a path's true length in cells and the cells written.  8 bytes.</summary>
    [StructLayout(LayoutKind.Sequential)]
    public struct NavPath
    {
        public int CellCount, WrittenCount;
    }

    /// <summary>slamhip_nav_summary (include/slamhip.h): the class map's rectangle, the traversable and the reached cells, the sources
    /// used and blocked, the largest cost reached and the relaxation rounds the device ran.  10 words, 40 bytes.</summary>
    [StructLayout(LayoutKind.Sequential)]
    public struct NavSummary
    {
        public int MapX0, MapY0, MapWidth, MapHeight;
        public int TraversableCount, ReachedCount;
        public int SourcesUsed, SourcesBlocked;
        public uint MaxCostReached;
        public int Rounds;
    }

    /// <summary>slamhip_rollout_result (include/slamhip.h): the leading free poses of one command rollout, the step and value of the
    /// least cost-to-go along them, the cost at the last free pose, and that pose.  7 words, 28 bytes, no padding.</summary>
    [StructLayout(LayoutKind.Sequential)]
    public struct RolloutResult
    {
        public const uint Unreached = 0xFFFFFFFFu;
        public int FreeCount, MinStep;
        public uint EndCost, MinCost;
        public float X, Y, Theta;
    }

    /// <summary>slamhip_rollout_summary (include/slamhip.h): the field's summary, the cost at the start pose, the complete rollouts
    /// and the two keys (cost &lt;&lt; 32 | b; NoKey: no rollout qualifies).  64 bytes, no padding.</summary>
    [StructLayout(LayoutKind.Sequential)]
    public struct RolloutSummary
    {
        public const ulong NoKey = 0xFFFFFFFFFFFFFFFFul;
        public NavSummary Nav;
        public uint StartCost;
        public int CompleteCount;
        public ulong KeyEnd, KeyMin;
    }

    /// <summary>slamhip_merge_report (include/slamhip.h): the destination cells of a merge counted by their class and their source
    /// cell's -- Joint(cd, cs), classes 0 neither, 1 occupied, 2 free -- those with no source cell, and what an apply changed and cut.
    /// 96 bytes, no padding.</summary>
    [StructLayout(LayoutKind.Sequential)]
    public unsafe struct MergeReport
    {
        public fixed long JointCounts[9];
        public long UnsourcedCount, ChangedCount, ClampedCount;
        public long Joint(int destinationClass, int sourceClass) => JointCounts[3 * destinationClass + sourceClass];
    }

    /// <summary>slamhip_hough_shift (include/slamhip.h): the row correlation of one pair -- the shift at its maximum (ties to the
    /// smallest), how many shifts reach it, the maximum and the sum over all shifts.  24 bytes, no padding.</summary>
    [StructLayout(LayoutKind.Sequential)]
    public struct HoughShift
    {
        public int BestShift, TieCount;
        public ulong BestValue, Sum;
    }

    /// <summary>slamhip_sig_spec (include/slamhip.h): the spec of the scan signatures -- cells per metre, the rings and the cells of a
    /// ring's width; 64 sectors always.  12 bytes.</summary>
    [StructLayout(LayoutKind.Sequential)]
    public struct SigSpec
    {
        public float Scale;
        public int RingCount, RingCells;
    }

    /// <summary>slamhip_sig_info (include/slamhip.h): the points of a scan, those ignored, those beyond the last ring, and the bits
    /// set in its signature.  16 bytes.</summary>
    [StructLayout(LayoutKind.Sequential)]
    public struct SigInfo
    {
        public int PointCount, IgnoredCount, FarCount, SetCount;
    }

    /// <summary>slamhip_sig_hit (include/slamhip.h): one keyframe a scan resembles -- the score (Jaccard index in 16.16, at most
    /// 65536), the keyframe's index (-1: none), the shift in sectors (the query's heading is the keyframe's minus Shift * 2 pi / 64),
    /// the common and the united bits and the keyframe's own.  16 bytes, no padding.</summary>
    [StructLayout(LayoutKind.Sequential)]
    public struct SigHit
    {
        public uint Score;
        public int Index;
        public short Shift, Inter, Union, KeySetCount;
    }

    /// <summary>slamhip_pg_spec (include/slamhip.h): the Gauss-Newton steps, the most PCG iterations of a step, the iterations enqueued
    /// between two reads of the stop word (no result depends on it), 0, lambda and the tolerance of rule 7.  32 bytes: four int32 at
    /// offsets 0, 4, 8, 12, two doubles at 16 and 24.</summary>
    [StructLayout(LayoutKind.Sequential)]
    public struct PgSpec
    {
        public int OuterCount, CgCount, CheckEvery, Reserved;
        public double Lambda, Tolerance;
    }

    /// <summary>slamhip_scanmatch_spec (include/slamhip.h): cells per metre, the raster's half side H (a multiple of 16 in [16, 192]),
    /// the lattice's half widths (each at most 64), the heading step, the margin of the near-optimal set, 0.  32 bytes.</summary>
    [StructLayout(LayoutKind.Sequential)]
    public struct ScanMatchSpec
    {
        public float Scale;
        public int Half, Nx, Ny, Nt;
        public float DTheta;
        public int Margin, Reserved;
    }

    /// <summary>slamhip_scan_pair: two indices into the scan store and the guess, the QUERY's pose in the REFERENCE's frame.  20 bytes.</summary>
    [StructLayout(LayoutKind.Sequential)]
    public struct ScanPair
    {
        public int Ref, Query;
        public Vector3 Guess;
    }

    /// <summary>slamhip_scanmatch_result: the best node and its score, the points that counted, the size of the near-optimal set and
    /// its nine integer moments.  104 bytes, no padding.</summary>
    [StructLayout(LayoutKind.Sequential)]
    public struct ScanMatchResult
    {
        public int K, Ix, Iy, Score, RefCount, QueryCount, Count, Reserved;
        public long SumX, SumY, SumK, SumXX, SumYY, SumKK, SumXY, SumXK, SumYK;
    }

    /// <summary>slamhip_pg_iter (include/slamhip.h): chi2 before the step, rz0, the last rz, the PCG iterations completed and why they
    /// stopped (0 tolerance reached, 1 CgCount reached, 2 breakdown).  32 bytes.</summary>
    [StructLayout(LayoutKind.Sequential)]
    public struct PgIter
    {
        public double Chi2, Rz0, Rz;
        public int CgIterations, Stopped;
    }

    /// <summary>slamhip_pg_lm_spec (include/slamhip.h): the attempts, the most PCG iterations of one, the iterations between two reads of
    /// the stop word, the preconditioner (0 block-Jacobi, 1 the odometry chain), the robust kernel (0 none, 1 DCS, 2 Geman-McClure), 0;
    /// the first lambda, its factors behind a rejected and an accepted attempt, its bounds, rule 7's tolerance, rule R3's, the kernel's
    /// phi.  88 bytes: six int32 from offset 0, eight doubles from offset 24.</summary>
    [StructLayout(LayoutKind.Sequential)]
    public struct PgLmSpec
    {
        public int OuterCount, CgCount, CheckEvery, Precond, Kind, Reserved;
        public double Lambda0, Up, Down, LambdaMin, LambdaMax, Tolerance, CostTolerance, Phi;
    }

    /// <summary>slamhip_pg_lm_iter (include/slamhip.h): the cost before the attempt and at its trial poses, the lambda it used, rz0, the
    /// last rz, the PCG iterations and why they stopped (as PgIter), whether the attempt was accepted, three reserved words.  64 bytes.</summary>
    [StructLayout(LayoutKind.Sequential)]
    public struct PgLmIter
    {
        public double Cost, TrialCost, Lambda, Rz0, Rz;
        public int CgIterations, Stopped, Accepted, Reserved0, Reserved1, Reserved2;
    }

    /// <summary>slamhip_pg_marg_spec (include/slamhip.h): the most PCG iterations of a right-hand side, the iterations between two reads of
    /// the stop words, the preconditioner (0 block-Jacobi, 1 the odometry chain), a reserved word, lambda, rule 7's tolerance and rule
    /// M5's bound of the work block in bytes (0: 256 MiB).  40 bytes.</summary>
    [StructLayout(LayoutKind.Sequential)]
    public struct PgMargSpec
    {
        public int CgCount, CheckEvery, Precond, Reserved;
        public double Lambda, Tolerance;
        public long MaxBytes;
    }

    /// <summary>slamhip_pg_marg_col (include/slamhip.h): one right-hand side e(Node, Component) of a marginals query: rz0, the last rz,
    /// the PCG iterations and why they stopped (as PgIter).  32 bytes.</summary>
    [StructLayout(LayoutKind.Sequential)]
    public struct PgMargCol
    {
        public double Rz0, Rz;
        public int CgIterations, Stopped, Node, Component;
    }

    /// <summary>slamhip_pg_marg_info (include/slamhip.h): the columns and right-hand sides of a query, the right-hand sides per chunk, the
    /// chunks, the group size of the kernels, three reserved words.  32 bytes.</summary>
    [StructLayout(LayoutKind.Sequential)]
    public struct PgMargInfo
    {
        public int Columns, RightHandSides, PerChunk, Chunks, Group, Reserved0, Reserved1, Reserved2;
    }

    /// <summary>What slamhip_hs_hough reports of the slot it filled: the map's size and first cell, D = w + h, the bins per angle N,
    /// the sites, and the spectrum HS (T entries); H (T rows of N) when asked for.</summary>
    public sealed class HoughInfo
    {
        public int W, H, X0, Y0, D, N, Sites, T, Q;
        public ulong[] Spectrum;
        public uint[] Votes;
    }

    /// <summary>slamhip_view_summary (include/slamhip.h): the DISTINCT cells one pose's beams see on a level -- the beams by status, the
    /// cut ones, the seen cells and their split by class, and those not in the covered layer.  Ten int32, 40 bytes, no padding.</summary>
    [StructLayout(LayoutKind.Sequential)]
    public struct ViewSummary
    {
        public int WalkedCount, SameCount, IgnoredCount;
        public int CutCount;
        public int SeenCount;
        public int UnknownCount, FreeCount, OccupiedCount;
        public int NewCount, NewUnknownCount;
    }

    /// <summary>slamhip_mcl_spec (include/slamhip.h): one particle-filter localisation step -- the field's level, world, site mask and
    /// radius, the odometry increment in the robot's frame, the noise scales, the window's movement since the last step, the weight
    /// scale, the resampling threshold and the Philox key and stream.  72 bytes, no padding.</summary>
    [StructLayout(LayoutKind.Sequential)]
    public struct MclSpec
    {
        public int Level, World, SiteMask, Radius;
        public float Dx, Dy, Dtheta;
        public float SigmaX, SigmaY, SigmaTheta;
        public float FrameOffsetX, FrameOffsetY;
        public uint Beta;
        public int MinEffectiveCount;
        public ulong Seed, Stream;
    }

    /// <summary>slamhip_mcl_summary (include/slamhip.h): the exact integer sums of one localisation step.  The effective sample size is
    /// A * A / Q; the weighted-mean pose (SumHx / A / 1024, SumHy / A / 1024, atan2(SumHs, SumHc)).  96 bytes, no padding.</summary>
    [StructLayout(LayoutKind.Sequential)]
    public struct MclSummary
    {
        public ulong W, A, Q, KeyBest;
        public long SumHx, SumHy, SumHc, SumHs;
        public ulong CostMin, CostMax;
        public int Resampled, DistinctCount, UnplacedCount, ParticleCount;
    }

    internal static unsafe class Native
    {
        const string Lib = "slamhip";                                   // libslamhip.so on the library path

        [DllImport(Lib)] internal static extern IntPtr slamhip_version();
        [DllImport(Lib)] internal static extern IntPtr slamhip_last_error();
        [DllImport(Lib)] internal static extern int slamhip_device_count(out int count);

        // ---- context: one GPU + one HIP stream; stands where `new ParallelWorker(n)` stood --------------------------
        [DllImport(Lib)] internal static extern int slamhip_ctx_create(int deviceOrdinal, out IntPtr ctx);
        [DllImport(Lib)] internal static extern int slamhip_ctx_destroy(IntPtr ctx);
        [DllImport(Lib)] internal static extern int slamhip_ctx_synchronize(IntPtr ctx);
        [DllImport(Lib)] internal static extern int slamhip_ctx_set_wait_timeout(IntPtr ctx, long timeoutMs);
        [DllImport(Lib)] internal static extern int slamhip_ctx_poisoned(IntPtr ctx, out int poisoned);
        [DllImport(Lib)] internal static extern int slamhip_ctx_philox4x32_10(IntPtr ctx, uint[] counter4, uint[] key2, [Out] uint[] out4);

        // ---- CoreSLAM operator level --------------------------------------------------------------------------------
        [DllImport(Lib)] internal static extern int slamhip_cs_create(IntPtr ctx, float physicalMapSize, int holeMapSize, int obstacleMapSize, out IntPtr cs);
        [DllImport(Lib)] internal static extern int slamhip_cs_destroy(IntPtr cs);
        [DllImport(Lib)] internal static extern int slamhip_cs_info(IntPtr cs, out int holeSize, out float holeScale, out int obstSize, out float obstScale);
        [DllImport(Lib)] internal static extern int slamhip_cs_reset(IntPtr cs, int unmappedObstacleHits);
        [DllImport(Lib)] internal static extern int slamhip_cs_holemap_upload(IntPtr cs, ushort* pixels, nuint n);
        [DllImport(Lib)] internal static extern int slamhip_cs_holemap_download(IntPtr cs, ushort* pixels, nuint n);
        [DllImport(Lib)] internal static extern int slamhip_cs_holemap_download_packed(IntPtr cs, byte* packed, nuint nBytes);
        [DllImport(Lib)] internal static extern int slamhip_cs_holemap_mirror(IntPtr cs, ushort* pixels, nuint n, int* rectX0Y0X1Y1);
        [DllImport(Lib)] internal static extern int slamhip_cs_holemap_mirror_async(IntPtr cs, ushort* pixels, nuint n);
        [DllImport(Lib)] internal static extern int slamhip_cs_holemap_mirror_wait(IntPtr cs, int* rectX0Y0X1Y1, long* pixelsPushed);
        [DllImport(Lib)] internal static extern int slamhip_cs_holemap_mirror_release(IntPtr cs);
        [DllImport(Lib)] internal static extern int slamhip_cs_obstaclemap_upload(IntPtr cs, sbyte* pixels, nuint n);
        [DllImport(Lib)] internal static extern int slamhip_cs_obstaclemap_download(IntPtr cs, sbyte* pixels, nuint n);
        [DllImport(Lib)] internal static extern int slamhip_cs_set_scan(IntPtr cs, Vector2* points, int nPoints);
        [DllImport(Lib)] internal static extern int slamhip_cs_distance_pxcs(IntPtr cs, Vector4* pxcs, int k, int* outDist, out int bestIndex, out int bestDist);
        [DllImport(Lib)] internal static extern int slamhip_cs_distance_poses(IntPtr cs, Vector3* poses, int k, int* outDist, out int bestIndex, out int bestDist);
        [DllImport(Lib)] internal static extern int slamhip_cs_set_offsets(IntPtr cs, Vector3* offs, int n);
        [DllImport(Lib)] internal static extern int slamhip_cs_generate_offsets(IntPtr cs, int n, float sigmaXY, float sigmaTheta, ulong seed, ulong stream);
        [DllImport(Lib)] internal static extern int slamhip_cs_generate_offsets_lattice(IntPtr cs, int n, float sigmaXY, float sigmaTheta, ulong seed, ulong stream);
        [DllImport(Lib)] internal static extern int slamhip_cs_prepared_lists(IntPtr cs, out ulong served, out ulong prepared);
        [DllImport(Lib)] internal static extern int slamhip_cs_prelaunch_stats(IntPtr cs, [Out] ulong[] four);
        [DllImport(Lib)] internal static extern int slamhip_cs_plan_stats(IntPtr cs, [Out] ulong[] four);
        [DllImport(Lib)] internal static extern int slamhip_cs_search(IntPtr cs, in Vector3 searchPose, out Vector3 pose, out int dist, out int index);
        [DllImport(Lib)] internal static extern int slamhip_cs_update_holemap(IntPtr cs, in Vector3 pose, float holeWidth, int quality);
        [DllImport(Lib)] internal static extern int slamhip_cs_update_holemap_pxcs(IntPtr cs, in Vector4 pxcs, float holeWidth, int quality);
        [DllImport(Lib)] internal static extern int slamhip_cs_update_obstaclemap(IntPtr cs, in Vector3 pose, int maxObstacleHits);
        [DllImport(Lib)] internal static extern int slamhip_cs_update_obstaclemap_pxcs(IntPtr cs, in Vector4 pxcs, int maxObstacleHits);
        [DllImport(Lib)] internal static extern int slamhip_cs_search_and_update(IntPtr cs, in Vector3 searchPose, float holeWidth, int quality, int maxObstacleHits,
                                                                                 out Vector3 pose, out int dist, out int index);
        [DllImport(Lib)] internal static extern int slamhip_cs_scan_search_and_update(IntPtr cs, Vector2* xy, int nPoints, in Vector3 searchPose, float holeWidth, int quality, int maxObstacleHits,
                                                                                      out Vector3 pose, out int dist, out int index);
        // the search report (slamhip.h: slamhip_search_report): the plain forms' results, the ordinary launch order
        [DllImport(Lib)] internal static extern int slamhip_cs_search_report(IntPtr cs, in Vector3 searchPose, int band, out Vector3 pose, out SearchReport report);
        [DllImport(Lib)] internal static extern int slamhip_cs_search_distances(IntPtr cs, int* dist, int k);
        [DllImport(Lib)] internal static extern int slamhip_cs_search_and_update_report(IntPtr cs, in Vector3 searchPose, int band, float holeWidth, int quality, int maxObstacleHits,
                                                                                        out Vector3 pose, out SearchReport report);
        [DllImport(Lib)] internal static extern int slamhip_cs_scan_search_and_update_report(IntPtr cs, Vector2* xy, int nPoints, in Vector3 searchPose, int band, float holeWidth, int quality,
                                                                                             int maxObstacleHits, out Vector3 pose, out SearchReport report);
        [DllImport(Lib)] internal static extern int slamhip_cs_search_and_update_pxcs(IntPtr cs, Vector4* pxcsSearch, Vector4* pxcsUpdateHole, Vector4* pxcsUpdateObstacle, int k,
                                                                                      float holeWidth, int quality, int maxObstacleHits, out int index, out int dist);
        [DllImport(Lib)] internal static extern int slamhip_cs_update_maps_pxcs(IntPtr cs, in Vector4 pxcsHole, in Vector4 pxcsObstacle, float holeWidth, int quality, int maxObstacleHits);
        [DllImport(Lib)] internal static extern int slamhip_cs_offsets_download(IntPtr cs, Vector3* offs, int n);

        // ---- HectorSLAM operator level ------------------------------------------------------------------------------
        [DllImport(Lib)] internal static extern int slamhip_hs_create(IntPtr ctx, float cellLength, int width, int height, int levels, out IntPtr hs);
        [DllImport(Lib)] internal static extern int slamhip_hs_destroy(IntPtr hs);
        [DllImport(Lib)] internal static extern int slamhip_hs_reset(IntPtr hs);
        [DllImport(Lib)] internal static extern int slamhip_hs_level_info(IntPtr hs, int level, out int width, out int height, out float cellLength);
        [DllImport(Lib)] internal static extern int slamhip_hs_set_factors(IntPtr hs, float free, float occupied);
        [DllImport(Lib)] internal static extern int slamhip_hs_set_iterations(IntPtr hs, int* perLevel);
        [DllImport(Lib)] internal static extern int slamhip_hs_cells_upload(IntPtr hs, int level, HectorSLAM.Map.LogOddsCell* cells, nuint n);
        [DllImport(Lib)] internal static extern int slamhip_hs_cells_download(IntPtr hs, int level, HectorSLAM.Map.LogOddsCell* cells, nuint n);
        [DllImport(Lib)] internal static extern int slamhip_hs_bitmap_download(IntPtr hs, int level, byte* data, nuint n);
        [DllImport(Lib)] internal static extern int slamhip_hs_map_extends(IntPtr hs, int level, int* xMaxYMaxXMinYMin, out int found);
        [DllImport(Lib)] internal static extern int slamhip_hs_probability(IntPtr hs, int level, int* indices, int n, float* p);
        [DllImport(Lib)] internal static extern int slamhip_hs_set_scan(IntPtr hs, Vector2* points, int nPoints, in Vector2 scanOrigin);
        [DllImport(Lib)] internal static extern int slamhip_hs_match(IntPtr hs, in Vector3 hint, out Vector3 pose);
        [DllImport(Lib)] internal static extern int slamhip_hs_match_level(IntPtr hs, int level, in Vector3 hint, int iterations, out Vector3 pose);
        [DllImport(Lib)] internal static extern int slamhip_hs_match_batch(IntPtr hs, Vector3* hints, int count, Vector3* poses);
        // ScanMatcher(numThreads)'s summation order (ScanMatcher.cs:149-195): 0 the device's own, 1..64 the reference's chunks, bit for bit
        [DllImport(Lib)] internal static extern int slamhip_hs_match_report(IntPtr hs, in Vector3 hint, out Vector3 pose, out MatchReport report);
        [DllImport(Lib)] internal static extern int slamhip_hs_match_level_report(IntPtr hs, int level, in Vector3 hint, int iterations, out Vector3 pose, out MatchReport report);
        [DllImport(Lib)] internal static extern int slamhip_hs_match_batch_report(IntPtr hs, Vector3* hints, int count, Vector3* poses, MatchReport* reports);
        [DllImport(Lib)] internal static extern int slamhip_hs_match_best(IntPtr hs, Vector3* hints, int count, out Vector3 pose, out int index, out MatchReport report);
        // relocalisation in a loaded map (no reference counterpart): the pose-lattice search, its node poses, and search + best-of-batch match
        [DllImport(Lib)] internal static extern int slamhip_hs_lattice_search(IntPtr hs, in LatticeSpec spec, ulong* keys, int* scores);
        [DllImport(Lib)] internal static extern int slamhip_hs_lattice_node_pose(IntPtr hs, in LatticeSpec spec, int k, int flat, out Vector3 pose);
        [DllImport(Lib)] internal static extern int slamhip_hs_relocalise(IntPtr hs, in LatticeSpec spec, int maxHints, out Vector3 pose, out MatchReport report, out RelocInfo info);
        [DllImport(Lib)] internal static extern int slamhip_hs_world_lattice_search(IntPtr hs, in LatticeSpec spec, ulong* keys, int* scores);
        [DllImport(Lib)] internal static extern int slamhip_hs_relocalise_world(IntPtr hs, in LatticeSpec spec, int maxHints, out Vector3 pose, out MatchReport report, out WorldRelocInfo info);
        [DllImport(Lib)] internal static extern int slamhip_debug_lattice_cells(float cellLength, in Vector3 centre, float theta, Vector2* xy, int n, int* gxgy);
        // the beam trace (no reference counterpart): the map along every beam of the scan, at many poses; and its host-side hooks
        [DllImport(Lib)] internal static extern int slamhip_hs_trace(IntPtr hs, int level, Vector3* poses, int nPoses, int world, TraceSummary* summaries, TraceBeam* beams);
        [DllImport(Lib)] internal static extern int slamhip_debug_trace_lines(float scaleToMap, in Vector3 pose, in Vector2 origin, Vector2* xy, int n, int* lines);
        [DllImport(Lib)] internal static extern int slamhip_debug_trace_cells(int bx, int by, int ex, int ey, int* cells, int cap, out int n);
        // the distance field and the end-point distance score (no reference counterpart), and the field's host-side hook
        [DllImport(Lib)] internal static extern int slamhip_hs_distance_field(IntPtr hs, int level, int world, int siteMask, int radius, int x, int y, int w, int h, ushort* d2);
        [DllImport(Lib)] internal static extern int slamhip_hs_distance_score(IntPtr hs, int level, int world, int siteMask, int radius, Vector3* poses, int nPoses,
                                                                              DistanceSummary* summaries, ushort* points);
        [DllImport(Lib)] internal static extern int slamhip_debug_distance_field(byte* cls, int cw, int ch, int siteMask, int radius, int x, int y, int w, int h, ushort* d2);
        // the nearest site of every cell and the scan-to-map pairs (no reference counterpart), and the field's host-side hook
        [DllImport(Lib)] internal static extern int slamhip_hs_nearest_field(IntPtr hs, int level, int world, int siteMask, int radius, int x, int y, int w, int h, short* dxdy);
        [DllImport(Lib)] internal static extern int slamhip_hs_nearest_pairs(IntPtr hs, int level, int world, int siteMask, int radius, Vector3* poses, int nPoses,
                                                                             PairSummary* summaries, short* pairs);
        // the Hough transform of a map, the rotation scores and the row correlations (no reference counterpart)
        [DllImport(Lib)] internal static extern int slamhip_hs_hough(IntPtr hs, int level, int slot, int world, int siteMask, int nAngles, int q, int* info7, ulong* spectrum, uint* votes);
        [DllImport(Lib)] internal static extern int slamhip_hs_hough_rotation(IntPtr hs, ulong* cc);
        [DllImport(Lib)] internal static extern int slamhip_hs_hough_shifts(IntPtr hs, int* pairs, int nPairs, HoughShift* shifts, ulong* xc);
        [DllImport(Lib)] internal static extern int slamhip_hs_hough_clear(IntPtr hs);
        // scan signatures and the keyframe store for loop candidates (no reference counterpart)
        [DllImport(Lib)] internal static extern int slamhip_hs_sig_configure(IntPtr hs, in SigSpec spec);
        [DllImport(Lib)] internal static extern int slamhip_hs_sig_add(IntPtr hs, in Vector3 pose, out int index, ulong* sig, out SigInfo info);
        [DllImport(Lib)] internal static extern int slamhip_hs_sig_add_scans(IntPtr hs, Vector2* points, int* offsets, int nScans, Vector3* poses, out int first);
        [DllImport(Lib)] internal static extern int slamhip_hs_sig_query(IntPtr hs, int first, int last, int maxHits, SigHit* hits, out int n, ulong* sig, out SigInfo info);
        [DllImport(Lib)] internal static extern int slamhip_hs_sig_self(IntPtr hs, int first, int last, int minGap, SigHit* hits);
        [DllImport(Lib)] internal static extern int slamhip_hs_sig_count(IntPtr hs, out int count);
        [DllImport(Lib)] internal static extern int slamhip_hs_sig_download(IntPtr hs, int first, int n, ulong* sig, Vector3* poses);
        [DllImport(Lib)] internal static extern int slamhip_hs_sig_upload(IntPtr hs, int n, ulong* sig, Vector3* poses);
        [DllImport(Lib)] internal static extern int slamhip_hs_sig_clear(IntPtr hs);
        [DllImport(Lib)] internal static extern int slamhip_hs_sig_set_poses(IntPtr hs, int first, int n, Vector3* poses);
        // relaxation of a pose graph of keyframes (no reference counterpart)
        [DllImport(Lib)] internal static extern int slamhip_hs_pg_set(IntPtr hs, double* poses, byte* isFixed, int nNodes, int* ij, double* z, double* w, int nEdges);
        [DllImport(Lib)] internal static extern int slamhip_hs_pg_relax(IntPtr hs, in PgSpec spec, PgIter* iters, out double chi2Final);
        [DllImport(Lib)] internal static extern int slamhip_hs_pg_relax_tri(IntPtr hs, in PgSpec spec, PgIter* iters, out double chi2Final);
        [DllImport(Lib)] internal static extern int slamhip_hs_pg_relax_lm(IntPtr hs, in PgLmSpec spec, byte* robust, PgLmIter* iters, out int count, out double costFinal, double* factors);
        [DllImport(Lib)] internal static extern int slamhip_hs_pg_marginals(IntPtr hs, in PgMargSpec spec, int* pairs, int nPairs, double* blocks, PgMargCol* cols, out int count, out PgMargInfo info);
        [DllImport(Lib)] internal static extern int slamhip_hs_pg_tri_apply(IntPtr hs, double lambda, double* rhs, double* z);
        [DllImport(Lib)] internal static extern int slamhip_hs_pg_get(IntPtr hs, double* poses, int nNodes);
        [DllImport(Lib)] internal static extern int slamhip_hs_pg_residuals(IntPtr hs, double* r, double* chi2);
        [DllImport(Lib)] internal static extern int slamhip_hs_pg_clear(IntPtr hs);
        [DllImport(Lib)] internal static extern int slamhip_hs_scans_add(IntPtr hs, Vector2* points, int nPoints, Vector2* scanOrigin, out int index);
        [DllImport(Lib)] internal static extern int slamhip_hs_scans_count(IntPtr hs, out int count);
        [DllImport(Lib)] internal static extern int slamhip_hs_scans_info(IntPtr hs, int k, out int nPoints, out Vector2 scanOrigin);
        [DllImport(Lib)] internal static extern int slamhip_hs_scans_download(IntPtr hs, int k, Vector2* points, int cap);
        [DllImport(Lib)] internal static extern int slamhip_hs_scans_clear(IntPtr hs);
        [DllImport(Lib)] internal static extern int slamhip_hs_render(IntPtr hs, int first, int last, Vector3* poses, int flags);
        // stored scans matched pairwise (no reference counterpart), the edge rule and the host-side hook
        [DllImport(Lib)] internal static extern int slamhip_hs_scans_match(IntPtr hs, in ScanMatchSpec spec, ScanPair* pairs, int nPairs, ScanMatchResult* results);
        [DllImport(Lib)] internal static extern int slamhip_hs_scans_edges(in ScanMatchSpec spec, ScanPair* pairs, ScanMatchResult* results, int n, double* z, double* w, int* valid);
        [DllImport(Lib)] internal static extern int slamhip_debug_scans_match(Vector2* points, int* offsets, int nScans, in ScanMatchSpec spec, ScanPair* pairs, int nPairs, ScanMatchResult* results);
        [DllImport(Lib)] internal static extern int slamhip_debug_nearest_field(byte* cls, int cw, int ch, int siteMask, int radius, int x, int y, int w, int h, short* dxdy);
        // the frontier cells and their connected clusters (no reference counterpart), and their host-side hook
        [DllImport(Lib)] internal static extern int slamhip_hs_frontiers(IntPtr hs, int level, int world, int minCells, int maxClusters, out FrontierSummary summary, FrontierCluster* clusters,
                                                                         int lx, int ly, int lw, int lh, int* labels);
        [DllImport(Lib)] internal static extern int slamhip_debug_frontiers(byte* cls, int cw, int ch, int minCells, int maxClusters, out FrontierSummary summary, FrontierCluster* clusters,
                                                                            int* labels);
        // the cost-to-go field, goal costs and paths (no reference counterpart), and their host-side hook
        [DllImport(Lib)] internal static extern int slamhip_hs_nav_field(IntPtr hs, ref NavSpec spec, int* sources, int nSources, int* goals, int nGoals, NavGoalResult* goalResults,
                                                                        int nPaths, int maxPathCells, NavPath* paths, int* pathCells, int rx, int ry, int rw, int rh, uint* cost, byte* dir,
                                                                        out NavSummary summary);
        [DllImport(Lib)] internal static extern int slamhip_hs_rollouts(IntPtr hs, ref NavSpec spec, int* sources, int nSources, float* startPose, float dt, float* body, int nBody,
                                                                       float* cmds, int nRollouts, int nCmd, int hold, RolloutResult* results, out RolloutSummary summary);
        [DllImport(Lib)] internal static extern int slamhip_hs_mcl_set(IntPtr hs, Vector3* poses, int nParticles);
        [DllImport(Lib)] internal static extern int slamhip_hs_mcl_step(IntPtr hs, in MclSpec spec, out MclSummary summary);
        [DllImport(Lib)] internal static extern int slamhip_hs_mcl_get(IntPtr hs, Vector3* poses, ulong* acc, int* ancestors, int nParticles);
        [DllImport(Lib)] internal static extern int slamhip_debug_mcl_step(byte* cls, int cw, int ch, float stm, Vector2* points, int nPoints, Vector3* particlesIn, ulong* accIn, int nParticles,
                                                                          in MclSpec spec, Vector3* particlesOut, ulong* accOut, int* ancestorsOut, out MclSummary summary);
        [DllImport(Lib)] internal static extern int slamhip_debug_mcl_table(uint* table64);
        [DllImport(Lib)] internal static extern int slamhip_hs_merge_set_source(IntPtr hs, int level, int ax, int ay, int w, int h, HectorSLAM.Map.LogOddsCell* cells);
        [DllImport(Lib)] internal static extern int slamhip_hs_merge_score(IntPtr hs, Vector3* poses, int nPoses, MergeReport* reports);
        [DllImport(Lib)] internal static extern int slamhip_hs_merge_apply(IntPtr hs, in Vector3 pose, int rule, float valueLimit, out MergeReport report);
        [DllImport(Lib)] internal static extern int slamhip_hs_merge_clear_source(IntPtr hs);
        [DllImport(Lib)] internal static extern int slamhip_debug_merge(HectorSLAM.Map.LogOddsCell* dst, int dw, int dh, HectorSLAM.Map.LogOddsCell* src, int ax, int ay, int sw, int sh, in Vector3 pose, float stm,
                                                                       int rule, float valueLimit, HectorSLAM.Map.LogOddsCell* cellsOut, out MergeReport report);
        [DllImport(Lib)] internal static extern int slamhip_debug_merge_box(in Vector3 pose, float stm, int ax, int ay, int sw, int sh, int x0, int y0, int x1, int y1, int* box4,
                                                                           out int any);
        // the view gain and the greedy choice of views (no reference counterpart), and their host-side hook
        [DllImport(Lib)] internal static extern int slamhip_hs_view_set_covered(IntPtr hs, int level, uint* bits);
        [DllImport(Lib)] internal static extern int slamhip_hs_view_get_covered(IntPtr hs, int level, uint* bits);
        [DllImport(Lib)] internal static extern int slamhip_hs_view_clear(IntPtr hs);
        [DllImport(Lib)] internal static extern int slamhip_hs_view_gain(IntPtr hs, int level, int reach, Vector3* poses, int nPoses, int commit, ViewSummary* summaries);
        [DllImport(Lib)] internal static extern int slamhip_hs_view_select(IntPtr hs, int level, int reach, int mode, int minGain, Vector3* poses, int nPoses, int k, int* order, int* gain,
                                                                           out int n);
        [DllImport(Lib)] internal static extern int slamhip_debug_view(float* values, int w, int h, float scaleToMap, in Vector3 pose, in Vector2 origin, Vector2* xy, int n, int reach,
                                                                       uint* covered, uint* bitsOut, out ViewSummary summary);
        [DllImport(Lib)] internal static extern int slamhip_debug_rollouts(byte* cls, int cw, int ch, int siteMask, int clearance, uint maxCost, int* sources, int nSources, float stm,
                                                                          float* startPose, float dt, float* body, int nBody, float* cmds, int nRollouts, int nCmd, int hold,
                                                                          RolloutResult* results, out RolloutSummary summary);
        [DllImport(Lib)] internal static extern int slamhip_debug_nav_field(byte* cls, int cw, int ch, int siteMask, int clearance, uint maxCost, int* sources, int nSources, int* goals,
                                                                           int nGoals, NavGoalResult* goalResults, int nPaths, int maxPathCells, NavPath* paths, int* pathCells, int rx,
                                                                           int ry, int rw, int rh, uint* cost, byte* dir, out NavSummary summary);
        [DllImport(Lib)] internal static extern int slamhip_hs_set_match_threads(IntPtr hs, int numThreads);
        [DllImport(Lib)] internal static extern int slamhip_hs_set_reference_cache(IntPtr hs, int on);
        [DllImport(Lib)] internal static extern int slamhip_hs_update_by_scan(IntPtr hs, in Vector3 robotPoseWorld);
        [DllImport(Lib)] internal static extern int slamhip_hs_shift(IntPtr hs, int dx, int dy);
        [DllImport(Lib)] internal static extern int slamhip_hs_origin(IntPtr hs, out long ox, out long oy);
        // the scrolling window's backing store: what scrolls out is kept in a device tile pool and restored on return (maxBytes 0 = off)
        [DllImport(Lib)] internal static extern int slamhip_hs_set_backing(IntPtr hs, int tileCells, ulong maxBytes);
        [DllImport(Lib)] internal static extern int slamhip_hs_backing_stats(IntPtr hs, out BackingStats stats);
        [DllImport(Lib)] internal static extern int slamhip_hs_world_cells_download(IntPtr hs, int level, long x0, long y0, int w, int h, HectorSLAM.Map.LogOddsCell* cells);
        // ... and back: the inverse of the world download (returns OK whatever the capacity; droppedCells counts what found no place), and the world's extents
        [DllImport(Lib)] internal static extern int slamhip_hs_world_cells_upload(IntPtr hs, int level, long x0, long y0, int w, int h, HectorSLAM.Map.LogOddsCell* cells, out long droppedCells);
        [DllImport(Lib)] internal static extern int slamhip_hs_world_extends(IntPtr hs, int level, long* xMaxYMaxXMinYMin, out int found);
        // HectorSLAM, processor level (HectorSLAMProcessor.cs:66-138): the Update state machine in the library -- match, the gate of :107-109 evaluated
        // on the device, the grid update enqueued behind the match before the pose is back (one blocking wait per scan instead of two)
        [DllImport(Lib)] internal static extern int slamhip_hsproc_create(IntPtr ctx, float mapResolution, int width, int height, in Vector3 startPose, int numDepth, out IntPtr proc);
        [DllImport(Lib)] internal static extern int slamhip_hsproc_destroy(IntPtr proc);
        [DllImport(Lib)] internal static extern int slamhip_hsproc_reset(IntPtr proc);
        [DllImport(Lib)] internal static extern int slamhip_hsproc_update(IntPtr proc, Vector2* points, int nPoints, in Vector2 scanOrigin, in Vector3 poseHintWorld, int mapWithoutMatching, out int mapUpdated);
        [DllImport(Lib)] internal static extern int slamhip_hsproc_get(IntPtr proc, out Vector3 matchPose, out Vector3 lastMapUpdatePose, out float matchTimingMs, out float updateTimingMs);
        [DllImport(Lib)] internal static extern int slamhip_hsproc_set_match_report(IntPtr proc, int on);
        [DllImport(Lib)] internal static extern int slamhip_hsproc_get_report(IntPtr proc, out MatchReport report, out int valid);
        [DllImport(Lib)] internal static extern int slamhip_hsproc_set_thresholds(IntPtr proc, float minDistanceDiff, float minAngleDiff);
        [DllImport(Lib)] internal static extern int slamhip_hsproc_hs(IntPtr proc, out IntPtr hs);
        [DllImport(Lib)] internal static extern int slamhip_hsproc_set_scroll(IntPtr proc, int triggerCells);
        [DllImport(Lib)] internal static extern int slamhip_hsproc_get_origin(IntPtr proc, out long ox, out long oy);
        [DllImport(Lib)] internal static extern int slamhip_hsproc_shift(IntPtr proc, int dx, int dy);
        [DllImport(Lib)] internal static extern int slamhip_hsproc_relocalise(IntPtr proc, Vector2* points, int nPoints, in Vector2 scanOrigin, in LatticeSpec specWorld, int maxHints, int adopt,
                                                                              out Vector3 poseWorld, out MatchReport report, out RelocInfo info);
        [DllImport(Lib)] internal static extern int slamhip_hsproc_trace(IntPtr proc, Vector2* points, int nPoints, in Vector2 scanOrigin, Vector3* posesWorld, int nPoses, int level, int world,
                                                                         TraceSummary* summaries, TraceBeam* beams);
        [DllImport(Lib)] internal static extern int slamhip_hsproc_distance_score(IntPtr proc, Vector2* points, int nPoints, in Vector2 scanOrigin, Vector3* posesWorld, int nPoses, int level, int world,
                                                                                  int siteMask, int radius, DistanceSummary* summaries, ushort* pointD2);
        [DllImport(Lib)] internal static extern int slamhip_hsproc_nearest_pairs(IntPtr proc, Vector2* points, int nPoints, in Vector2 scanOrigin, Vector3* posesWorld, int nPoses, int level, int world,
                                                                                 int siteMask, int radius, PairSummary* summaries, short* pairs);
        [DllImport(Lib)] internal static extern int slamhip_hsproc_hough(IntPtr proc, int level, int slot, int world, int siteMask, int nAngles, int q, int* info7, ulong* spectrum, uint* votes);
        [DllImport(Lib)] internal static extern int slamhip_hsproc_hough_rotation(IntPtr proc, ulong* cc);
        [DllImport(Lib)] internal static extern int slamhip_hsproc_hough_shifts(IntPtr proc, int* pairs, int nPairs, HoughShift* shifts, ulong* xc);
        [DllImport(Lib)] internal static extern int slamhip_hsproc_sig_add(IntPtr proc, Vector2* points, int nPoints, in Vector2 scanOrigin, in Vector3 poseWorld, out int index, ulong* sig,
                                                                           out SigInfo info);
        [DllImport(Lib)] internal static extern int slamhip_hsproc_sig_query(IntPtr proc, Vector2* points, int nPoints, in Vector2 scanOrigin, int first, int last, int maxHits, SigHit* hits,
                                                                             out int n, ulong* sig, out SigInfo info);
        [DllImport(Lib)] internal static extern int slamhip_hsproc_sig_self(IntPtr proc, int first, int last, int minGap, SigHit* hits);
        [DllImport(Lib)] internal static extern int slamhip_hsproc_scans_add(IntPtr proc, out int index);
        [DllImport(Lib)] internal static extern int slamhip_hsproc_render(IntPtr proc, int first, int last, Vector3* poses, int flags);
        [DllImport(Lib)] internal static extern int slamhip_hsproc_scans_match(IntPtr proc, in ScanMatchSpec spec, ScanPair* pairs, int nPairs, ScanMatchResult* results);
        [DllImport(Lib)] internal static extern int slamhip_hsproc_mcl_step(IntPtr proc, Vector2* points, int nPoints, in Vector2 scanOrigin, in MclSpec spec, out MclSummary summary);
        [DllImport(Lib)] internal static extern int slamhip_hsproc_merge_set_source(IntPtr proc, int level, int ax, int ay, int w, int h, HectorSLAM.Map.LogOddsCell* cells);
        [DllImport(Lib)] internal static extern int slamhip_hsproc_merge_score(IntPtr proc, Vector3* posesWorld, int nPoses, MergeReport* reports);
        [DllImport(Lib)] internal static extern int slamhip_hsproc_merge_apply(IntPtr proc, in Vector3 poseWorld, int rule, float valueLimit, out MergeReport report);
        [DllImport(Lib)] internal static extern int slamhip_hsproc_view_gain(IntPtr proc, Vector2* points, int nPoints, in Vector2 scanOrigin, Vector3* posesWorld, int nPoses, int level, int reach,
                                                                             int commit, ViewSummary* summaries);
        [DllImport(Lib)] internal static extern int slamhip_hsproc_view_select(IntPtr proc, Vector2* points, int nPoints, in Vector2 scanOrigin, Vector3* posesWorld, int nPoses, int level, int reach,
                                                                               int mode, int minGain, int k, int* order, int* gain, out int n);
        [DllImport(Lib)] internal static extern int slamhip_hsproc_frontiers(IntPtr proc, int level, int world, int minCells, int maxClusters, out FrontierSummary summary, FrontierCluster* clusters,
                                                                             int lx, int ly, int lw, int lh, int* labels);
        [DllImport(Lib)] internal static extern int slamhip_hsproc_rollouts(IntPtr proc, ref NavSpec spec, int* sources, int nSources, float* startPoseWorld, float dt, float* body, int nBody,
                                                                           float* cmds, int nRollouts, int nCmd, int hold, RolloutResult* results, out RolloutSummary summary);
        [DllImport(Lib)] internal static extern int slamhip_hsproc_nav_field(IntPtr proc, ref NavSpec spec, int* sources, int nSources, int* goals, int nGoals, NavGoalResult* goalResults,
                                                                            int nPaths, int maxPathCells, NavPath* paths, int* pathCells, int rx, int ry, int rw, int rh, uint* cost,
                                                                            byte* dir, out NavSummary summary);
        [DllImport(Lib)] internal static extern int slamhip_hsproc_relocalise_world(IntPtr proc, Vector2* points, int nPoints, in Vector2 scanOrigin, in LatticeSpec specWorld, int maxHints, int adopt,
                                                                                    out Vector3 poseWorld, out MatchReport report, out WorldRelocInfo info);

        // ---- one process, several GPUs -------------------------------------------------------------------------------
        [DllImport(Lib)] internal static extern int slamhip_group_create(int* deviceOrdinals, int n, float physicalMapSize, int holeMapSize, int obstacleMapSize, out IntPtr group);
        [DllImport(Lib)] internal static extern int slamhip_group_destroy(IntPtr group);
        [DllImport(Lib)] internal static extern int slamhip_group_cs(IntPtr group, int rank, out IntPtr cs);
        [DllImport(Lib)] internal static extern int slamhip_group_reset(IntPtr group, int unmappedObstacleHits);
        [DllImport(Lib)] internal static extern int slamhip_group_set_scan(IntPtr group, Vector2* points, int nPoints);
        [DllImport(Lib)] internal static extern int slamhip_group_set_offsets(IntPtr group, Vector3* offs, int n);
        [DllImport(Lib)] internal static extern int slamhip_group_generate_offsets(IntPtr group, int n, float sigmaXY, float sigmaTheta, ulong seed, ulong stream);
        [DllImport(Lib)] internal static extern int slamhip_group_size(IntPtr group, out int n);
        [DllImport(Lib)] internal static extern int slamhip_group_holemap_upload(IntPtr group, ushort* pixels, nuint n);
        [DllImport(Lib)] internal static extern int slamhip_group_search_and_update(IntPtr group, in Vector3 searchPose, float holeWidth, int quality, int maxObstacleHits,
                                                                                    out Vector3 pose, out int dist, out int index);
        [DllImport(Lib)] internal static extern int slamhip_group_search(IntPtr group, in Vector3 searchPose, out Vector3 pose, out int dist, out int index);
        [DllImport(Lib)] internal static extern int slamhip_group_update_maps(IntPtr group, in Vector3 pose, float holeWidth, int quality, int maxObstacleHits);
        [DllImport(Lib)] internal static extern int slamhip_group_replicas_equal(IntPtr group, out int equal);
        [DllImport(Lib)] internal static extern int slamhip_cs_maps_checksum(IntPtr cs, ulong* holeAndObstacleWords);
        [DllImport(Lib)] internal static extern int slamhip_hs_checksum(IntPtr hs, int level, ulong* valueAndUpdateIndexWords);

        internal const int ErrTimeout = -6;                              // SLAMHIP_ERR_TIMEOUT: a blocking wait passed its bound; the context is poisoned

        internal static void Check(int status)
        {
            if (status == ErrTimeout)
                throw new TimeoutException($"slamhip: {Marshal.PtrToStringAnsi(slamhip_last_error())} (the device context is poisoned: dispose the objects on it)");
            if (status != 0)
                throw new InvalidOperationException($"slamhip error {status}: {Marshal.PtrToStringAnsi(slamhip_last_error())}");
        }
    }

    /// <summary>Owner of one native handle (slamhip_ctx / _cs / _hs): Dispose or finalisation calls its *_destroy.</summary>
    internal sealed class Handle : SafeHandle
    {
        private readonly Func<IntPtr, int> destroy;

        internal Handle(IntPtr h, Func<IntPtr, int> destroy) : base(IntPtr.Zero, true)
        {
            SetHandle(h);
            this.destroy = destroy;
        }

        public override bool IsInvalid => handle == IntPtr.Zero;

        internal IntPtr Ptr => handle;

        protected override bool ReleaseHandle() => destroy(handle) == 0;
    }

    /// <summary>One GPU and one HIP stream.  A processor owns one; pass a shared one to put several objects on the same device.</summary>
    public sealed class Device : IDisposable
    {
        internal readonly Handle Ctx;

        public int Ordinal { get; }

        public Device(int ordinal = 0)
        {
            Native.Check(Native.slamhip_ctx_create(ordinal, out IntPtr h));
            Ctx = new Handle(h, Native.slamhip_ctx_destroy);
            Ordinal = ordinal;
        }

        public static int Count
        {
            get { Native.Check(Native.slamhip_device_count(out int n)); return n; }
        }

        public void Synchronize() => Native.Check(Native.slamhip_ctx_synchronize(Ctx.Ptr));

        /// <summary>Bound on every blocking wait on this device, in milliseconds (default 10 000, or SLAMHIP_WAIT_TIMEOUT_MS; 0: none).
        /// The reference's ParallelWorker.Work waits for its threads without a bound; here a kernel that never ends surfaces as a
        /// TimeoutException, after which the device context is poisoned: every later call fails at once, nothing is re-executed, and
        /// the objects on it are to be disposed.</summary>
        public long WaitTimeoutMs
        {
            set => Native.Check(Native.slamhip_ctx_set_wait_timeout(Ctx.Ptr, value));
        }

        /// <summary>True once a blocking wait on this device has timed out.</summary>
        public bool Poisoned
        {
            get { Native.Check(Native.slamhip_ctx_poisoned(Ctx.Ptr, out int p)); return p != 0; }
        }

        public void Dispose() => Ctx.Dispose();
    }
}
