// HectorSLAM.Main.HectorSLAMProcessor over the library's own processor (reference: HectorSLAM/Main/HectorSLAMProcessor.cs:17-160):
// match against the pyramid, then redraw the maps only if the robot moved or turned enough.  Update is ONE native call
// (slamhip_hsproc_update): the library matches, evaluates the gate of :107-109 on the device with the float operations the reference
// applies on the host, and enqueues the grid update behind the match before the pose is back -- one blocking wait per scan (round 5
// measured 56 us per Update that way against two blocking calls, match 37.5 us + update, from managed code).  MapRep is the processor's
// own pyramid (slamhip_hsproc_hs), so everything a caller reads from it (cells, bitmaps, extends) is what Update wrote.
using System;
using System.Drawing;
using System.Numerics;
using System.Runtime.InteropServices;
using BaseSLAM;
using Microsoft.Extensions.Logging;
using SlamHip;

namespace HectorSLAM.Main
{
    public class HectorSLAMProcessor : IDisposable
    {
        private readonly ILogger logger;
        private readonly Device device;
        private readonly bool ownsDevice;
        private readonly Handle proc;
        private readonly int numThreads;
        private float minDistanceDiff = 0.3f, minAngleDiff = 0.13f;
        private bool referenceSummation;
        private bool matchReport;
        private int scrollTrigger;

        public MapRepMultiMap MapRep { get; private set; }
        public Vector3 LastMapUpdatePose { get; private set; }
        public Vector3 MatchPose { get; private set; }
        /// <summary>Moving average of the matching time, ms (HectorSLAMProcessor.cs:41,96; kept by the library).</summary>
        public float MatchTiming { get; private set; }
        /// <summary>Moving average of the map update time, ms (:46,115): the update is enqueued, not waited for, so this is the enqueue.</summary>
        public float UpdateTiming { get; private set; }

        public float MinDistanceDiffForMapUpdate                          // :51
        {
            get => minDistanceDiff;
            set { minDistanceDiff = value; Native.Check(Native.slamhip_hsproc_set_thresholds(proc.Ptr, minDistanceDiff, minAngleDiff)); }
        }

        public float MinAngleDiffForMapUpdate                             // :56
        {
            get => minAngleDiff;
            set { minAngleDiff = value; Native.Check(Native.slamhip_hsproc_set_thresholds(proc.Ptr, minDistanceDiff, minAngleDiff)); }
        }

        /// <summary>Match in the reference's summation order for the constructor's numThreads (1..64): the matcher's H, dTr and
        /// poses are then ScanMatcher(numThreads)'s bits (ScanMatcher.cs:149-195; slamhip_hs_set_match_threads on MapRep).
        /// false (default): the device's own order, poses within 1e-4 m / 1e-4 rad of the reference's.</summary>
        public bool ReferenceSummation
        {
            get => referenceSummation;
            set
            {
                if (value && (numThreads < 1 || numThreads > 64))
                    throw new InvalidOperationException("reference summation needs 1..64 threads");
                Native.Check(Native.slamhip_hs_set_match_threads(MapRep.Pyramid.Ptr, value ? numThreads : 0));
                referenceSummation = value;
            }
        }

        /// <summary>Match through the reference's probability cache (MapRep.ReferenceCache; slamhip_hs_set_reference_cache): with
        /// ReferenceSummation, Update then gives the reference's poses also across Reset, where its cache serves pre-reset
        /// probabilities (OccGridMap.cs:97-107,248).  false (default): the current probabilities (deviation D5).</summary>
        public bool ReferenceCache
        {
            get => MapRep.ReferenceCache;
            set => MapRep.ReferenceCache = value;
        }

        /// <summary>Every Update's match leaves its report (slamhip_hsproc_set_match_report), produced in the match's own launch;
        /// poses, the gated map update and what Update returns do not change.  false (default): Update launches what it always did.</summary>
        public bool MatchReport
        {
            get => matchReport;
            set { Native.Check(Native.slamhip_hsproc_set_match_report(proc.Ptr, value ? 1 : 0)); matchReport = value; }
        }

        /// <summary>Keep the robot in the window (slamhip_hsproc_set_scroll): 0 (default) off; > 0: at the end of an Update whose match
        /// pose lies more than this many level-0 cells from the window's middle on an axis, the pyramid is shifted on the device
        /// (MapRepMultiMap.Shift) so that the pose is back near the middle.  Hints, MatchPose and LastMapUpdatePose stay world poses;
        /// Origin says where the window lies.  Valid: 0 .. min(width, height) / 2 - (1 << (numDepth - 1)) - 1.</summary>
        public int ScrollTrigger
        {
            get => scrollTrigger;
            set { Native.Check(Native.slamhip_hsproc_set_scroll(proc.Ptr, value)); scrollTrigger = value; }
        }

        /// <summary>Keep what ScrollTrigger moves out of the window (MapRep.SetBacking; slamhip_hs_set_backing on the processor's own
        /// pyramid): (tileCells, maxBytes), or null (default) for off -- a robot that drives a loop then comes home to the map it made.</summary>
        public (int TileCells, ulong MaxBytes)? ScrollBacking
        {
            get => scrollBacking;
            set
            {
                if (value.HasValue) MapRep.SetBacking(value.Value.TileCells, value.Value.MaxBytes);
                else MapRep.SetBacking(0, 0);
                scrollBacking = value.HasValue && value.Value.MaxBytes > 0 ? value : null;
            }
        }
        private (int TileCells, ulong MaxBytes)? scrollBacking;

        /// <summary>The window's origin in level-0 cells (slamhip_hsproc_get_origin): the sum of all shifts since the last Reset.</summary>
        public (long X, long Y) Origin
        {
            get
            {
                Native.Check(Native.slamhip_hsproc_get_origin(proc.Ptr, out long ox, out long oy));
                return (ox, oy);
            }
        }

        /// <summary>The report of the last Update's match, or null: before the first match, after Reset, after an Update with
        /// mapWithoutMatching, and while MatchReport is off.</summary>
        public SlamHip.MatchReport? LastMatchReport { get; private set; }   // (qualified: MatchReport alone is the property above)

        public HectorSLAMProcessor(float mapResolution, Point mapSize, Vector3 startPose, int numDepth, int numThreads, ILogger logger = null)
            : this(mapResolution, mapSize, startPose, numDepth, numThreads, logger, null)
        {
        }

        /// <param name="numThreads">the reference's matcher threads (:72); the device needs none, and sums in their order only with ReferenceSummation</param>
        public HectorSLAMProcessor(float mapResolution, Point mapSize, Vector3 startPose, int numDepth, int numThreads, ILogger logger, Device device)
        {
            this.logger = logger;
            this.numThreads = numThreads;
            this.device = device ?? new Device(0);
            ownsDevice = device == null;
            Native.Check(Native.slamhip_hsproc_create(this.device.Ctx.Ptr, mapResolution, mapSize.X, mapSize.Y, startPose, numDepth, out IntPtr h));
            proc = new Handle(h, Native.slamhip_hsproc_destroy);
            Native.Check(Native.slamhip_hsproc_hs(proc.Ptr, out IntPtr pyramid));
            MapRep = new MapRepMultiMap(this.device, pyramid, numDepth);
            Refresh();
        }

        /// <returns>true if the maps were redrawn (HectorSLAMProcessor.cs:86-126)</returns>
        public unsafe bool Update(ScanCloud scan, Vector3 poseHintWorld, bool mapWithoutMatching = false)
        {
            int updated;
            fixed (Vector2* p = CollectionsMarshal.AsSpan(scan.Points))
                Native.Check(Native.slamhip_hsproc_update(proc.Ptr, p, scan.Points.Count, new Vector2(scan.Pose.X, scan.Pose.Y), poseHintWorld,
                                                          mapWithoutMatching ? 1 : 0, out updated));
            Refresh();
            if (scrollTrigger != 0) MapRep.MarkStale();                  // (a shift moves the maps whether or not this scan redrew them)
            if (updated == 0) return false;
            MapRep.MarkStale();
            logger?.LogInformation($"Map update at {MatchPose.X:F3} {MatchPose.Y:F3} {MatchPose.Z:F4}");
            return true;
        }

        /// <summary>The processor's world -- window and tiles -- as one file (MapRep.SaveWorld).</summary>
        public void SaveWorld(string path)
        {
            MapRep.SaveWorld(path);
        }

        /// <summary>Resume from a saved world (MapRep.LoadWorld): construct the processor with startPose = the saved pose, LoadWorld,
        /// Update.  The window moves through slamhip_hsproc_shift, so MatchPose and LastMapUpdatePose stay the world poses they
        /// were.  Returns the cells dropped.</summary>
        public long LoadWorld(string path)
        {
            long dropped = MapRep.LoadWorld(path, (dx, dy) => Native.Check(Native.slamhip_hsproc_shift(proc.Ptr, dx, dy)));
            Refresh();
            return dropped;
        }

        /// <summary>Find the robot in the map the window holds (slamhip_hsproc_relocalise; the reference can only Reset): the scan is
        /// scored against level lattice.Level at every node of the lattice around lattice's centre, a WORLD pose, and the best nodes
        /// of the maxHints highest-scoring headings are refined by the matcher; the winner is returned with its match report.
        /// adopt: the pose becomes MatchPose and LastMapUpdatePose -- the next Update matches from it and redraws the map only once
        /// the robot has moved by the thresholds.  The resume flow: LoadWorld, Relocalise, Update.  The library sets no acceptance
        /// threshold: whether report.Residual is good enough is the caller's decision.</summary>
        public unsafe Vector3 Relocalise(ScanCloud scan, LatticeSpec lattice, int maxHints, bool adopt, out SlamHip.MatchReport report, out RelocInfo info)
        {
            Vector3 pose;
            fixed (Vector2* p = CollectionsMarshal.AsSpan(scan.Points))
                Native.Check(Native.slamhip_hsproc_relocalise(proc.Ptr, p, scan.Points.Count, new Vector2(scan.Pose.X, scan.Pose.Y), lattice, maxHints, adopt ? 1 : 0,
                                                              out pose, out report, out info));
            Refresh();
            return pose;
        }

        /// <summary>Relocalise over the whole saved world (slamhip_hsproc_relocalise_world; backing must be on): the lattice is scored
        /// against the window and the tiles behind it, the window then moves to the best node (info.Dx, info.Dy) and the matcher
        /// refines there.  Poses stay world poses.  The resume flow: LoadWorld, RelocaliseWorld, Update.</summary>
        public unsafe Vector3 RelocaliseWorld(ScanCloud scan, LatticeSpec lattice, int maxHints, bool adopt, out SlamHip.MatchReport report, out WorldRelocInfo info)
        {
            Vector3 pose;
            fixed (Vector2* p = CollectionsMarshal.AsSpan(scan.Points))
                Native.Check(Native.slamhip_hsproc_relocalise_world(proc.Ptr, p, scan.Points.Count, new Vector2(scan.Pose.X, scan.Pose.Y), lattice, maxHints, adopt ? 1 : 0,
                                                                    out pose, out report, out info));
            Refresh();
            return pose;
        }

        /// <summary>MapRep.Trace of `scan` at WORLD poses (slamhip_hsproc_trace): what the map of `level` holds along every beam, per
        /// pose a summary and, when asked for, the beam records [pose][beam], whose Hx, Hy stay window-frame cells of the level
        /// (world cell = (Origin >> level) + cell).  MatchPose, LastMapUpdatePose and the update gate are untouched.</summary>
        public unsafe TraceSummary[] Trace(ScanCloud scan, Vector3[] posesWorld, int level, bool world, bool wantBeams, out TraceBeam[] beams)
        {
            var sums = new TraceSummary[posesWorld.Length];
            beams = wantBeams ? new TraceBeam[(long)posesWorld.Length * scan.Points.Count] : null;
            fixed (Vector2* p = CollectionsMarshal.AsSpan(scan.Points))
            fixed (Vector3* q = posesWorld)
            fixed (TraceSummary* s = sums)
            fixed (TraceBeam* b = beams)
                Native.Check(Native.slamhip_hsproc_trace(proc.Ptr, p, scan.Points.Count, new Vector2(scan.Pose.X, scan.Pose.Y), q, posesWorld.Length, level, world ? 1 : 0, s, b));
            return sums;
        }

        /// <summary>MapRep.DistanceScore of `scan` at WORLD poses (slamhip_hsproc_distance_score): per pose how far the scan's end
        /// points lie from the sites of `level` (siteMask 2: mapped obstacles), in squared cells capped at radius^2, and when asked
        /// for the values [pose][point].  MatchPose, LastMapUpdatePose and the update gate are untouched.</summary>
        public unsafe DistanceSummary[] DistanceScore(ScanCloud scan, Vector3[] posesWorld, int level, int siteMask, int radius, bool world, bool wantPoints, out ushort[] points)
        {
            var sums = new DistanceSummary[posesWorld.Length];
            points = wantPoints ? new ushort[(long)posesWorld.Length * scan.Points.Count] : null;
            fixed (Vector2* p = CollectionsMarshal.AsSpan(scan.Points))
            fixed (Vector3* q = posesWorld)
            fixed (DistanceSummary* s = sums)
            fixed (ushort* d = points)
                Native.Check(Native.slamhip_hsproc_distance_score(proc.Ptr, p, scan.Points.Count, new Vector2(scan.Pose.X, scan.Pose.Y), q, posesWorld.Length, level, world ? 1 : 0,
                                                                  siteMask, radius, s, d));
            return sums;
        }

        /// <summary>MapRep.NearestPairs of `scan` at WORLD poses (slamhip_hsproc_nearest_pairs): per pose the nearest site of `level`
        /// (siteMask 2: mapped obstacles) within `radius` cells of every end cell, as counts and the sums an alignment step needs --
        /// in window-frame cells -- and when asked for the offsets [2 * (pose * points + point)].  MatchPose, LastMapUpdatePose and
        /// the update gate are untouched.</summary>
        public unsafe PairSummary[] NearestPairs(ScanCloud scan, Vector3[] posesWorld, int level, int siteMask, int radius, bool world, bool wantPairs, out short[] pairs)
        {
            var sums = new PairSummary[posesWorld.Length];
            pairs = wantPairs ? new short[2 * (long)posesWorld.Length * scan.Points.Count] : null;
            fixed (Vector2* p = CollectionsMarshal.AsSpan(scan.Points))
            fixed (Vector3* q = posesWorld)
            fixed (PairSummary* s = sums)
            fixed (short* d = pairs)
                Native.Check(Native.slamhip_hsproc_nearest_pairs(proc.Ptr, p, scan.Points.Count, new Vector2(scan.Pose.X, scan.Pose.Y), q, posesWorld.Length, level, world ? 1 : 0,
                                                                 siteMask, radius, s, d));
            return sums;
        }

        /// <summary>One point-to-map alignment step of `scan` at a WORLD pose: NearestPairs there, then MapRepMultiMap.AlignStep --
        /// host arithmetic only -- on the pose in the window's frame (minus (float)Origin * Maps[0].CellLength per axis, as the
        /// library takes it), handed back as a world pose.  Iteration is the caller's loop: call again with the result until
        /// summary.ZeroCount == summary.MatchedCount or the step is small enough.  Nothing of the processor changes.</summary>
        public Vector3 AlignStep(ScanCloud scan, Vector3 poseWorld, int level, out PairSummary summary, int siteMask = 2, int radius = 32, bool world = false)
        {
            summary = NearestPairs(scan, new[] { poseWorld }, level, siteMask, radius, world, false, out _)[0];
            float stm = 1.0f / MapRep.Maps[level].Properties.CellLength;
            var (ox, oy) = Origin;
            if (ox == 0 && oy == 0) return MapRepMultiMap.AlignStep(poseWorld, summary, stm);
            float cell0 = MapRep.Maps[0].Properties.CellLength;
            return MapRepMultiMap.AlignStep(new Vector3(poseWorld.X - (float)ox * cell0, poseWorld.Y - (float)oy * cell0, poseWorld.Z), summary, stm, poseWorld);
        }

        /// <summary>MapRep.Frontiers in WORLD cells of `level` (slamhip_hsproc_frontiers): seeds, boxes, sums and the summary's map
        /// rectangle are world cells.  centroids receives each cluster's centre in metres, world frame: the mean cell taken to the
        /// window's frame of the level, through the level's cell-to-world transform (cell * CellLength) and back by (float)Origin *
        /// Maps[0].CellLength as every world pose is.  No scan is needed; MatchPose, LastMapUpdatePose and the update gate are
        /// untouched.</summary>
        public unsafe FrontierCluster[] Frontiers(int level, out FrontierSummary summary, out Vector2[] centroids, int minCells = 1, int maxClusters = 256, bool world = false)
        {
            var rec = new FrontierCluster[Math.Max(maxClusters, 0)];
            fixed (FrontierCluster* c = rec)
                Native.Check(Native.slamhip_hsproc_frontiers(proc.Ptr, level, world ? 1 : 0, minCells, maxClusters, out summary, c, 0, 0, 0, 0, null));
            Array.Resize(ref rec, summary.ReturnedCount);
            var (ox, oy) = Origin;
            double cell = MapRep.Maps[level].Properties.CellLength;
            float cell0 = MapRep.Maps[0].Properties.CellLength;
            centroids = new Vector2[rec.Length];
            for (int i = 0; i < rec.Length; i++)
            {
                long n = rec[i].CellCount;                               // (the sums back in the window's frame: integers, exact)
                centroids[i] = new Vector2((float)((rec[i].SumX - n * (ox >> level)) / (double)n * cell + (double)((float)ox * cell0)),
                                           (float)((rec[i].SumY - n * (oy >> level)) / (double)n * cell + (double)((float)oy * cell0)));
            }
            return rec;
        }

        /// <summary>MapRep.NavField in WORLD cells of `spec.Level` (slamhip_hsproc_nav_field): sources, goals and rect are world cells,
        /// and so are the goals' cells, the paths and the summary's map rectangle.  No scan is needed; MatchPose, LastMapUpdatePose and
        /// the update gate are untouched.</summary>
        public unsafe NavGoalResult[] NavField(NavSpec spec, int[] sources, int[] goals, out NavSummary summary, int nPaths, int maxPathCells,
                                               out NavPath[] heads, out int[][] paths)
        {
            int nGoals = goals == null ? 0 : goals.Length / 4;
            var res = new NavGoalResult[nGoals];
            heads = new NavPath[Math.Max(nPaths, 0)];
            var cells = new int[2L * Math.Max(nPaths, 0) * Math.Max(maxPathCells, 0)];
            fixed (int* s = sources)
            fixed (int* g = goals)
            fixed (NavGoalResult* gr = res)
            fixed (NavPath* h = heads)
            fixed (int* pc = cells)
                Native.Check(Native.slamhip_hsproc_nav_field(proc.Ptr, ref spec, s, sources.Length / 2, g, nGoals, gr, nPaths, maxPathCells, h, pc, 0, 0, 0, 0, null, null, out summary));
            paths = MapRepMultiMap.NavPaths(heads, cells, maxPathCells);
            return res;
        }

        /// <summary>Which frontier to drive to: Frontiers, then NavField from the cell of MatchPose with each returned cluster's
        /// bounding box, grown by `grow` cells on every side, as a goal (the box, not the cluster's own cells).  Returns the clusters,
        /// reachable ones first by cost ascending (equal costs in Frontiers' order), the unreachable ones behind them in Frontiers' order;
        /// results[i] belongs to the i-th returned cluster.  Composition only: no device work of its own.</summary>
        public FrontierCluster[] ExploreGoals(int level, int clearance, out NavGoalResult[] results, int siteMask = 2, int minCells = 1, int maxClusters = 256, int grow = 0)
        {
            var rec = Frontiers(level, out _, out _, minCells, maxClusters);
            results = new NavGoalResult[rec.Length];
            if (rec.Length == 0) return rec;
            var goals = new int[4 * rec.Length];
            for (int i = 0; i < rec.Length; i++)
            {
                goals[4 * i] = rec[i].XMin - grow; goals[4 * i + 1] = rec[i].YMin - grow;
                goals[4 * i + 2] = rec[i].XMax + grow; goals[4 * i + 3] = rec[i].YMax + grow;
            }
            double cell = MapRep.Maps[level].Properties.CellLength;
            var pose = MatchPose;
            var source = new[] { (int)Math.Round(pose.X / cell, MidpointRounding.ToEven), (int)Math.Round(pose.Y / cell, MidpointRounding.ToEven) };
            var spec = new NavSpec { Level = level, World = 0, SiteMask = siteMask, Clearance = clearance, MaxCost = 0 };
            var res = NavField(spec, source, goals, out _, 0, 1, out _, out _);
            var order = new int[rec.Length];
            for (int i = 0; i < order.Length; i++) order[i] = i;
            Array.Sort(order, (a, b) => res[a].Cost != res[b].Cost ? res[a].Cost.CompareTo(res[b].Cost) : a.CompareTo(b));
            var sorted = new FrontierCluster[rec.Length];
            for (int i = 0; i < order.Length; i++) { sorted[i] = rec[order[i]]; results[i] = res[order[i]]; }
            return sorted;
        }

        /// <summary>MapRep.Rollouts in WORLD cells and the WORLD pose (slamhip_hsproc_rollouts): sources are world cells of
        /// `spec.Level`, startPose a world pose (null: MatchPose), cmds nRollouts * nCmd pairs (v, w), body pairs of metres in the
        /// robot's frame (null: none).  The results' poses and the summary's map rectangle are world values.  No scan is needed;
        /// MatchPose, LastMapUpdatePose and the update gate are untouched.</summary>
        public unsafe RolloutResult[] Rollouts(NavSpec spec, int[] sources, Vector3? startPose, float dt, float[] body, float[] cmds, int nCmd, int hold,
                                               out RolloutSummary summary)
        {
            int n = nCmd > 0 ? cmds.Length / (2 * nCmd) : 0;
            var res = new RolloutResult[Math.Max(n, 0)];
            var start = stackalloc float[3];
            if (startPose.HasValue) { start[0] = startPose.Value.X; start[1] = startPose.Value.Y; start[2] = startPose.Value.Z; }
            fixed (int* s = sources)
            fixed (float* b = body)
            fixed (float* c = cmds)
            fixed (RolloutResult* r = res)
                Native.Check(Native.slamhip_hsproc_rollouts(proc.Ptr, ref spec, s, sources.Length / 2, startPose.HasValue ? start : null, dt, b, body == null ? 0 : body.Length / 2,
                                                            c, n, nCmd, hold, r, out summary));
            return res;
        }

        /// <summary>The source map of the merge through the processor (slamhip_hsproc_merge_set_source): as MapRep.MergeSetSource.</summary>
        public unsafe void MergeSetSource(int level, int ax, int ay, int w, int h, HectorSLAM.Map.LogOddsCell[] cells)
        {
            if (cells.Length != w * h) throw new ArgumentException("cells must hold w * h elements");
            fixed (HectorSLAM.Map.LogOddsCell* c = cells)
                Native.Check(Native.slamhip_hsproc_merge_set_source(proc.Ptr, level, ax, ay, w, h, c));
        }

        /// <summary>MapRep.MergeScore at WORLD poses of the source frame's origin (slamhip_hsproc_merge_score).</summary>
        public unsafe MergeReport[] MergeScore(Vector3[] posesWorld)
        {
            var reports = new MergeReport[posesWorld.Length];
            fixed (Vector3* p = posesWorld)
            fixed (MergeReport* r = reports)
                Native.Check(Native.slamhip_hsproc_merge_score(proc.Ptr, p, posesWorld.Length, r));
            return reports;
        }

        /// <summary>MapRep.MergeApply at a WORLD pose (slamhip_hsproc_merge_apply).  MatchPose, LastMapUpdatePose and the update gate are
        /// untouched.</summary>
        public MergeReport MergeApply(Vector3 poseWorld, int rule, float valueLimit)
        {
            Native.Check(Native.slamhip_hsproc_merge_apply(proc.Ptr, poseWorld, rule, valueLimit, out MergeReport report));
            return report;
        }

        /// <summary>MapRep.Hough through the processor (slamhip_hsproc_hough): cells and bins, no pose to convert.</summary>
        public HoughInfo Hough(int level, int slot = 0, bool world = false, int siteMask = 2, int nAngles = 360, int q = 1, bool wantVotes = false)
            => MapRep.HoughCall(true, proc.Ptr, level, slot, world, siteMask, nAngles, q, wantVotes);

        /// <summary>MapRep.HoughRotation through the processor (slamhip_hsproc_hough_rotation).</summary>
        public unsafe ulong[] HoughRotation()
        {
            if (MapRep.HoughSlots[0] == null) throw new InvalidOperationException("fill both slots (Hough) first");
            var cc = new ulong[MapRep.HoughSlots[0].T];
            fixed (ulong* c = cc)
                Native.Check(Native.slamhip_hsproc_hough_rotation(proc.Ptr, c));
            return cc;
        }

        /// <summary>MapRep.HoughShifts through the processor (slamhip_hsproc_hough_shifts).</summary>
        public unsafe HoughShift[] HoughShifts(int[] pairs)
        {
            var res = new HoughShift[pairs.Length / 2];
            fixed (int* p = pairs)
            fixed (HoughShift* r = res)
                Native.Check(Native.slamhip_hsproc_hough_shifts(proc.Ptr, p, res.Length, r, null));
            return res;
        }

        /// <summary>One loop candidate: the hit and the pose guess (x_k, y_k, theta_k - Shift * 2 pi / 64) from the keyframe's stored
        /// WORLD pose.</summary>
        public struct LoopCandidate { public SigHit Hit; public Vector3 PoseGuess; }

        /// <summary>The signature of `scan` appended to the keyframe store with its WORLD pose (slamhip_hsproc_sig_add;
        /// MapRep.SigConfigure first).  MatchPose, LastMapUpdatePose and the update gate are untouched.</summary>
        public unsafe int AddKeyframe(ScanCloud scan, Vector3 poseWorld)
        {
            int index;
            fixed (Vector2* p = CollectionsMarshal.AsSpan(scan.Points))
                Native.Check(Native.slamhip_hsproc_sig_add(proc.Ptr, p, scan.Points.Count, new Vector2(scan.Pose.X, scan.Pose.Y), poseWorld, out index, null, out _));
            return index;
        }

        /// <summary>The keyframes `scan` resembles most over all 64 headings (slamhip_hsproc_sig_query over [0, count -
        /// excludeRecent)), higher score first.  Candidates only: VerifyLoop checks one against the map.</summary>
        public unsafe LoopCandidate[] LoopCandidates(ScanCloud scan, int maxHits = 16, int excludeRecent = 0)
        {
            var hits = new SigHit[16];
            int n, last = Math.Max(MapRep.SigCount - excludeRecent, 0);
            fixed (Vector2* p = CollectionsMarshal.AsSpan(scan.Points))
            fixed (SigHit* h = hits)
                Native.Check(Native.slamhip_hsproc_sig_query(proc.Ptr, p, scan.Points.Count, new Vector2(scan.Pose.X, scan.Pose.Y), 0, last, maxHits, h, out n, null, out _));
            var res = new LoopCandidate[n];
            for (int i = 0; i < n; i++)
            {
                MapRep.SigDownload(hits[i].Index, 1, out _, out Vector3[] pose);
                double th = Math.IEEERemainder(pose[0].Z - hits[i].Shift * 2.0 * Math.PI / 64.0, 2.0 * Math.PI);
                if (th <= -Math.PI) th += 2.0 * Math.PI;
                res[i] = new LoopCandidate { Hit = hits[i], PoseGuess = new Vector3(pose[0].X, pose[0].Y, (float)th) };
            }
            return res;
        }

        /// <summary>MapRep.SigSelf through the processor (slamhip_hsproc_sig_self).</summary>
        public unsafe SigHit[] SelfLoopCandidates(int first, int last, int minGap)
        {
            var hits = new SigHit[Math.Max(last - first, 1)];
            fixed (SigHit* h = hits)
                Native.Check(Native.slamhip_hsproc_sig_self(proc.Ptr, first, last, minGap, h));
            Array.Resize(ref hits, Math.Max(last - first, 0));
            return hits;
        }

        /// <summary>The scan that is set on the processor's pyramid -- the one the last Update or AddKeyframe took -- appended to the
        /// scan store (slamhip_hsproc_scans_add): call it right after AddKeyframe, the two stores' indices then agree.</summary>
        public int KeepKeyframeScan()
        {
            Native.Check(Native.slamhip_hsproc_scans_add(proc.Ptr, out int index));
            return index;
        }

        /// <summary>Draw the stored keyframe scans [first, last) into the map at WORLD poses -- those RelaxKeyframes returned -- in one
        /// call (slamhip_hsproc_render).  Without keep the map is cleared first.  MatchPose, LastMapUpdatePose and the gate stay.</summary>
        public unsafe void RenderKeyframes(Vector3[] posesWorld, int first, int last, bool keep = false)
        {
            Vector3[] p = posesWorld != null && posesWorld.Length > 0 ? posesWorld : new Vector3[1];
            fixed (Vector3* pp = p) Native.Check(Native.slamhip_hsproc_render(proc.Ptr, first, last, pp, keep ? 1 : 0));
        }

        /// <summary>Check one loop candidate against the map: Relocalise centred on its pose guess, nothing adopted.  Host
        /// composition only; the caller judges the report.</summary>
        public Vector3 VerifyLoop(ScanCloud scan, LoopCandidate candidate, LatticeSpec lattice, int maxHints, out SlamHip.MatchReport report, out RelocInfo info)
        {
            lattice.CentreX = candidate.PoseGuess.X; lattice.CentreY = candidate.PoseGuess.Y; lattice.CentreTheta = candidate.PoseGuess.Z;
            return Relocalise(scan, lattice, maxHints, false, out report, out info);
        }

        /// <summary>One verified loop for RelaxKeyframes: keyframe J seen in keyframe I's frame at Z = (x, y, theta), with the diagonal
        /// weights W, as the caller derives them from VerifyLoop.</summary>
        public struct LoopEdge { public int I, J; public Vector3 Z, W; }

        /// <summary>Spread verified loops over the keyframe store's poses: nodes are the stored poses, an odometry edge joins every
        /// pair of consecutive keyframes (its measurement formed from their stored poses, odomW its weights), one more edge per loop,
        /// node 0 fixed; then MapRep.PgSet, PgRelax, PgGet, PgResiduals and SigSetPoses.  Host composition only.  Returns the relaxed
        /// poses as they were written back to the store; chi2 holds the odometry edges first, then the loops.</summary>
        public Vector3[] RelaxKeyframes(LoopEdge[] loops, Vector3 odomW, PgSpec spec, out PgIter[] iters, out double[] chi2)
        {
            int n = MapRep.SigCount, e = Math.Max(n - 1, 0) + loops.Length;
            MapRep.SigDownload(0, n, out _, out Vector3[] kp);
            var poses = new double[3 * n]; var ij = new int[2 * e]; var z = new double[3 * e]; var w = new double[3 * e];
            for (int k = 0; k < n; k++) { poses[3 * k] = kp[k].X; poses[3 * k + 1] = kp[k].Y; poses[3 * k + 2] = kp[k].Z; }
            for (int k = 0; k + 1 < n; k++)
            {
                double c = Math.Cos(poses[3 * k + 2]), s = Math.Sin(poses[3 * k + 2]);
                double dx = poses[3 * k + 3] - poses[3 * k], dy = poses[3 * k + 4] - poses[3 * k + 1];
                ij[2 * k] = k; ij[2 * k + 1] = k + 1;
                z[3 * k] = c * dx + s * dy; z[3 * k + 1] = c * dy - s * dx;
                z[3 * k + 2] = Math.IEEERemainder(poses[3 * k + 5] - poses[3 * k + 2], 2.0 * Math.PI);
                w[3 * k] = odomW.X; w[3 * k + 1] = odomW.Y; w[3 * k + 2] = odomW.Z;
            }
            for (int l = 0, k = Math.Max(n - 1, 0); l < loops.Length; l++, k++)
            {
                ij[2 * k] = loops[l].I; ij[2 * k + 1] = loops[l].J;
                z[3 * k] = loops[l].Z.X; z[3 * k + 1] = loops[l].Z.Y; z[3 * k + 2] = loops[l].Z.Z;
                w[3 * k] = loops[l].W.X; w[3 * k + 1] = loops[l].W.Y; w[3 * k + 2] = loops[l].W.Z;
            }
            MapRep.PgSet(poses, null, ij, z, w);
            iters = MapRep.PgRelax(spec, out _);
            double[] relaxed = MapRep.PgGet();
            MapRep.PgResiduals(out _, out chi2);
            var res = new Vector3[n];
            for (int k = 0; k < n; k++) res[k] = new Vector3((float)relaxed[3 * k], (float)relaxed[3 * k + 1], (float)relaxed[3 * k + 2]);
            MapRep.SigSetPoses(0, res);
            return res;
        }

        /// <summary>MapRep.ScansMatch through the processor (slamhip_hsproc_scans_match): relative poses, no frame to convert.</summary>
        public unsafe ScanMatchResult[] ScansMatch(ScanMatchSpec spec, ScanPair[] pairs)
        {
            var res = new ScanMatchResult[Math.Max(pairs.Length, 1)];
            ScanPair[] pr = pairs.Length > 0 ? pairs : new ScanPair[1];
            fixed (ScanPair* p = pr) fixed (ScanMatchResult* r = res)
                Native.Check(Native.slamhip_hsproc_scans_match(proc.Ptr, spec, p, pairs.Length, r));
            Array.Resize(ref res, pairs.Length);
            return res;
        }

        /// <summary>Close the loops of the keyframe store (host composition; KeepKeyframeScan after every AddKeyframe first):
        /// SelfLoopCandidates names one candidate per keyframe, its guess (0, 0, -Shift 2 pi / 64) by K18's sign rule; ScansMatch and
        /// MapRepMultiMap.ScansEdges turn the candidates into edges (keyframe hit.Index to keyframe i); accept, the caller's predicate
        /// over a result's Score, QueryCount and Count, filters them -- the library sets no threshold; RelaxKeyframes adds the
        /// odometry edges, relaxes and writes the poses back; with render the stored scans are drawn again at them.  Returns the
        /// accepted edges; relaxed is null when there is none.</summary>
        public LoopEdge[] CloseLoops(int minGap, ScanMatchSpec spec, Func<ScanMatchResult, bool> accept, Vector3 odomW, PgSpec pg, bool render, out Vector3[] relaxed)
        {
            relaxed = null;
            int n = MapRep.SigCount;
            SigHit[] hits = SelfLoopCandidates(0, n, minGap);
            var pairs = new System.Collections.Generic.List<ScanPair>();
            for (int i = 0; i < hits.Length; i++)
            {
                if (hits[i].Index < 0) continue;
                float th = (float)Math.IEEERemainder(-hits[i].Shift * 2.0 * Math.PI / 64.0, 2.0 * Math.PI);
                pairs.Add(new ScanPair { Ref = hits[i].Index, Query = i, Guess = new Vector3(0f, 0f, th) });
            }
            if (pairs.Count == 0) return new LoopEdge[0];
            ScanPair[] pr = pairs.ToArray();
            ScanMatchResult[] res = ScansMatch(spec, pr);
            MapRepMultiMap.ScansEdges(spec, pr, res, out double[] z, out double[] w, out bool[] valid);
            var loops = new System.Collections.Generic.List<LoopEdge>();
            for (int k = 0; k < pr.Length; k++)
                if (valid[k] && accept(res[k]))
                    loops.Add(new LoopEdge { I = pr[k].Ref, J = pr[k].Query, Z = new Vector3((float)z[3 * k], (float)z[3 * k + 1], (float)z[3 * k + 2]),
                                             W = new Vector3((float)w[3 * k], (float)w[3 * k + 1], (float)w[3 * k + 2]) });
            if (loops.Count == 0) return new LoopEdge[0];
            relaxed = RelaxKeyframes(loops.ToArray(), odomW, pg, out _, out _);
            if (render) RenderKeyframes(relaxed, 0, n);
            return loops.ToArray();
        }

        /// <summary>One hypothesis of AlignMaps: the rotation index m (theta = m pi / T), the WORLD pose of the source frame, and its
        /// merge report.</summary>
        public struct MapAlignment { public int M; public Vector3 PoseWorld; public MergeReport Report; }

        /// <summary>Align the merge source (MergeSetSource first) with the window's map of its level WITHOUT a scan, by the Hough
        /// spectrum: both slots filled, the rotation scores' best nRot peaks, each at m and m + T (the pi ambiguity), two row
        /// correlations per hypothesis in ONE HoughShifts call (rows ka = arg-max HS_d and ka + T/2), the translation from the two
        /// shifts (MapRepMultiMap.HoughPose) and every hypothesis rated by MergeScore.  Ordered by Report.Joint(1, 1) (occupied on
        /// occupied) descending, then by index.  Host composition; the library forms no threshold and picks no peak.</summary>
        public MapAlignment[] AlignMaps(int level, int nAngles = 360, int q = 1, int nRot = 4, int siteMask = 2)
        {
            HoughInfo d = Hough(level, 0, false, siteMask, nAngles, q), s = Hough(level, 1, false, siteMask, nAngles, q);
            int T = nAngles;
            int[] peaks = MapRepMultiMap.HoughPeaks(HoughRotation(), nRot);
            int ka = 0;
            for (int k = 1; k < T; k++) if (d.Spectrum[k] > d.Spectrum[ka]) ka = k;    // (lowest index on ties)
            int kb = (ka + T / 2) % T;
            var ms = new int[2 * peaks.Length];
            var pairs = new int[8 * peaks.Length];
            for (int i = 0; i < ms.Length; i++) {
                ms[i] = peaks[i / 2] + (i % 2) * T;
                pairs[4 * i] = ms[i]; pairs[4 * i + 1] = ka; pairs[4 * i + 2] = ms[i]; pairs[4 * i + 3] = kb;
            }
            HoughShift[] recs = HoughShifts(pairs);
            float stm = 1.0f / MapRep.Maps[level].Properties.CellLength;
            var (ox, oy) = Origin;
            float cell0 = MapRep.Maps[0].Properties.CellLength;
            float offX = ox == 0 && oy == 0 ? 0.0f : (float)ox * cell0, offY = ox == 0 && oy == 0 ? 0.0f : (float)oy * cell0;
            var poses = new Vector3[ms.Length];
            for (int i = 0; i < ms.Length; i++) {
                Vector3 w = MapRepMultiMap.HoughPose(ms[i], recs[2 * i], ka, recs[2 * i + 1], kb, d, s, stm);
                poses[i] = new Vector3(w.X + offX, w.Y + offY, w.Z);
            }
            MergeReport[] reports = MergeScore(poses);
            var order = new int[ms.Length];
            for (int i = 0; i < order.Length; i++) order[i] = i;
            Array.Sort(order, (a, b) => reports[a].Joint(1, 1) != reports[b].Joint(1, 1) ? reports[b].Joint(1, 1).CompareTo(reports[a].Joint(1, 1)) : a.CompareTo(b));
            var res = new MapAlignment[ms.Length];
            for (int i = 0; i < res.Length; i++) res[i] = new MapAlignment { M = ms[order[i]], PoseWorld = poses[order[i]], Report = reports[order[i]] };
            return res;
        }

        /// <summary>MapRep.ViewGain of `scan` at WORLD poses (slamhip_hsproc_view_gain), taken to the window's frame as Trace takes them.
        /// MatchPose, LastMapUpdatePose and the update gate are untouched.</summary>
        public unsafe ViewSummary[] ViewGain(ScanCloud scan, Vector3[] posesWorld, int level, int reach, int commit = -1)
        {
            var sums = new ViewSummary[posesWorld.Length];
            fixed (Vector2* p = CollectionsMarshal.AsSpan(scan.Points))
            fixed (Vector3* q = posesWorld)
            fixed (ViewSummary* s = sums)
                Native.Check(Native.slamhip_hsproc_view_gain(proc.Ptr, p, scan.Points.Count, new Vector2(scan.Pose.X, scan.Pose.Y), q, posesWorld.Length, level, reach, commit, s));
            return sums;
        }

        /// <summary>MapRep.ViewSelect of `scan` at WORLD poses (slamhip_hsproc_view_select).</summary>
        public unsafe int[] ViewSelect(ScanCloud scan, Vector3[] posesWorld, int level, int reach, int k, int mode, int minGain, out int[] gains)
        {
            var order = new int[k];
            var gain = new int[k];
            int n;
            fixed (Vector2* p = CollectionsMarshal.AsSpan(scan.Points))
            fixed (Vector3* q = posesWorld)
            fixed (int* o = order)
            fixed (int* g = gain)
                Native.Check(Native.slamhip_hsproc_view_select(proc.Ptr, p, scan.Points.Count, new Vector2(scan.Pose.X, scan.Pose.Y), q, posesWorld.Length, level, reach, mode, minGain, k,
                                                               o, g, out n));
            Array.Resize(ref order, n);
            Array.Resize(ref gain, n);
            gains = gain;
            return order;
        }

        /// <summary>Start Monte-Carlo localisation: the particle set of the processor's own pyramid (MapRep.MclSet) from WORLD poses, taken
        /// to the window's frame as Relocalise takes its centre (minus (float)Origin * Maps[0].CellLength per axis).</summary>
        public void LocaliseInit(Vector3[] posesWorld)
        {
            var (ox, oy) = Origin;
            float cell0 = MapRep.Maps[0].Properties.CellLength;
            var p = (Vector3[])posesWorld.Clone();
            if (ox != 0 || oy != 0)
                for (int i = 0; i < p.Length; i++) { p[i].X = p[i].X - (float)ox * cell0; p[i].Y = p[i].Y - (float)oy * cell0; }
            MapRep.MclSet(p);
            mclOrigin = (ox, oy);
        }
        private (long X, long Y) mclOrigin;

        /// <summary>One localisation step (slamhip_hsproc_mcl_step): spec's odometry increment is in the robot's frame; its frame offset
        /// is set here to minus the window's movement since the last step.  Returns the weighted-mean pose in the world frame;
        /// effectiveCount = A * A / Q.  MatchPose, LastMapUpdatePose, the update gate and the map are untouched; the caller advances
        /// spec.Stream per step.</summary>
        public unsafe Vector3 LocaliseStep(ScanCloud scan, MclSpec spec, out double effectiveCount, out MclSummary summary)
        {
            var (ox, oy) = Origin;
            float cell0 = MapRep.Maps[0].Properties.CellLength;
            spec.FrameOffsetX = -((float)(ox - mclOrigin.X) * cell0); spec.FrameOffsetY = -((float)(oy - mclOrigin.Y) * cell0);
            fixed (Vector2* p = CollectionsMarshal.AsSpan(scan.Points))
                Native.Check(Native.slamhip_hsproc_mcl_step(proc.Ptr, p, scan.Points.Count, new Vector2(scan.Pose.X, scan.Pose.Y), spec, out summary));
            mclOrigin = (ox, oy);
            double a = summary.A;
            effectiveCount = a * a / summary.Q;
            return new Vector3((float)(summary.SumHx / a / 1024.0 + (double)((float)ox * cell0)), (float)(summary.SumHy / a / 1024.0 + (double)((float)oy * cell0)),
                               (float)Math.Atan2(summary.SumHs, summary.SumHc));
        }

        /// <summary>Which constant command to drive: Rollouts of the outer product of vValues and wValues (command b = (v[b / nw], w[b %
        /// nw]), nCmd = 1, hold = steps) towards goalCells (world cells).  Returns false when no rollout has a free pose; else the
        /// command decoded from KeyEnd -- the complete rollout that ends cheapest, fromEnd = true -- or, if nothing completes, from
        /// KeyMin, with its record.  Composition only: no device work of its own.</summary>
        public bool DriveCommand(int level, int[] goalCells, int clearance, float[] vValues, float[] wValues, float dt, int steps, float[] body,
                                 out float v, out float w, out bool fromEnd, out RolloutResult result, out RolloutSummary summary, int siteMask = 2)
        {
            var cmds = new float[2 * vValues.Length * wValues.Length];
            for (int i = 0; i < vValues.Length; i++)
                for (int j = 0; j < wValues.Length; j++) { cmds[2 * (i * wValues.Length + j)] = vValues[i]; cmds[2 * (i * wValues.Length + j) + 1] = wValues[j]; }
            var spec = new NavSpec { Level = level, World = 0, SiteMask = siteMask, Clearance = clearance, MaxCost = 0 };
            var res = Rollouts(spec, goalCells, null, dt, body, cmds, 1, steps, out summary);
            fromEnd = summary.KeyEnd != RolloutSummary.NoKey;
            ulong key = fromEnd ? summary.KeyEnd : summary.KeyMin;
            v = w = 0f; result = default;
            if (key == RolloutSummary.NoKey) return false;
            int b = (int)(key & 0xFFFFFFFFul);
            v = cmds[2 * b]; w = cmds[2 * b + 1]; result = res[b];
            return true;
        }

        private void Refresh()
        {
            Native.Check(Native.slamhip_hsproc_get(proc.Ptr, out Vector3 match, out Vector3 last, out float tm, out float tu));
            MatchPose = match; LastMapUpdatePose = last; MatchTiming = tm; UpdateTiming = tu;
            Native.Check(Native.slamhip_hsproc_get_report(proc.Ptr, out SlamHip.MatchReport report, out int valid));
            LastMatchReport = valid != 0 ? report : (SlamHip.MatchReport?)null;
        }

        public void Reset()                                              // :131-138
        {
            Native.Check(Native.slamhip_hsproc_reset(proc.Ptr));
            MapRep.MarkStale();
            Refresh();
        }

        public void Dispose()
        {
            MapRep.Dispose();                                            // (borrows the pyramid: nothing native is released here)
            proc.Dispose();
            if (ownsDevice) device.Dispose();
            GC.SuppressFinalize(this);
        }
    }
}
