// HectorSLAM.Main.MapRepMultiMap on the GPU (reference: HectorSLAM/Main/MapRepMultiMap.cs:19-97): level i has
// size / 2^i cells of resolution * 2^i metres; the levels are independent maps drawn from the same scan.  All levels live
// in ONE native pyramid and are updated by one pair of launches (the reference runs a Parallel.ForEach over them, :76).
using System;
using System.Drawing;
using System.Numerics;
using System.Runtime.InteropServices;
using BaseSLAM;
using HectorSLAM.Map;
using SlamHip;

namespace HectorSLAM.Main
{
    public class MapRepMultiMap : IDisposable
    {
        internal readonly Device Device;
        private readonly bool ownsDevice;
        internal readonly Handle Pyramid;

        public int NumLevels => Maps.Length;

        public OccGridMap[] Maps { get; }

        /// <param name="startCoords">must be Vector2.Zero (the only value the reference passes, HectorSLAMProcessor.cs:71)</param>
        public MapRepMultiMap(float mapResolution, Point mapSize, int numDepth, Vector2 startCoords, Device device = null)
        {
            if (startCoords != Vector2.Zero)
                throw new NotSupportedException("the device maps have no offset: move the window with MapRepMultiMap.Shift (slamhip_hs_shift)");
            Device = device ?? new Device(0);
            ownsDevice = device == null;
            Native.Check(Native.slamhip_hs_create(Device.Ctx.Ptr, mapResolution, mapSize.X, mapSize.Y, numDepth, out IntPtr h));
            Pyramid = new Handle(h, Native.slamhip_hs_destroy);
            Maps = new OccGridMap[numDepth];
            for (int i = 0; i < numDepth; i++)
            {
                Maps[i] = new OccGridMap(Device, Pyramid, i);
                Maps[i].IterationsChanged = PushIterations;
                Maps[i].FactorsChanged = () => { };                     // per-level factor setters exist for source compatibility; the pyramid's factors are set below
            }
            PushIterations();
        }

        /// <summary>The pyramid of a native HectorSLAMProcessor (slamhip_hsproc_hs): borrowed, the processor destroys it.</summary>
        internal MapRepMultiMap(Device device, IntPtr borrowedPyramid, int numDepth)
        {
            Device = device;
            ownsDevice = false;
            Pyramid = new Handle(borrowedPyramid, _ => 0);
            Maps = new OccGridMap[numDepth];
            for (int i = 0; i < numDepth; i++)
            {
                Maps[i] = new OccGridMap(Device, Pyramid, i);
                Maps[i].IterationsChanged = PushIterations;
                Maps[i].FactorsChanged = () => { };
            }
            PushIterations();
        }

        private unsafe void PushIterations()
        {
            int* it = stackalloc int[Maps.Length];
            for (int i = 0; i < Maps.Length; i++) it[i] = Maps[i] != null ? Maps[i].EstimateIterations : 3;
            Native.Check(Native.slamhip_hs_set_iterations(Pyramid.Ptr, it));
        }

        private bool referenceCache;

        /// <summary>Serve probabilities through OccGridMap's own cache (OccGridMap.cs:16,97-107; slamhip_hs_set_reference_cache):
        /// the matcher and GetCachedProbability then read what the reference reads, including the pre-reset values its cache
        /// keeps across Reset (:248).  Every switch to true starts from a new OccGridMap's cache.  false (default): the current
        /// probability of every cell (deviation D5).</summary>
        public bool ReferenceCache
        {
            get => referenceCache;
            set
            {
                Native.Check(Native.slamhip_hs_set_reference_cache(Pyramid.Ptr, value ? 1 : 0));
                referenceCache = value;
            }
        }

        public void Reset()                                              // MapRepMultiMap.cs:63-66
        {
            Native.Check(Native.slamhip_hs_reset(Pyramid.Ptr));
            foreach (OccGridMap m in Maps) m.mirrorStale = true;
        }

        /// <summary>Every level from the same scan (MapRepMultiMap.cs:73-77).</summary>
        public unsafe void UpdateByScan(ScanCloud scan, Vector3 pose)
        {
            SetScan(scan);
            Native.Check(Native.slamhip_hs_update_by_scan(Pyramid.Ptr, pose));
            foreach (OccGridMap m in Maps) m.mirrorStale = true;
        }

        /// <summary>Move the window by (+dx, +dy) level-0 cells on the device, in stream order (slamhip_hs_shift): on level l new cell
        /// (x, y) holds what old cell (x + (dx >> l), y + (dy >> l)) held, and exposed cells are LogOddsCell.Reset().  dx and dy must be
        /// multiples of 1 << (NumLevels - 1).  MatchData and UpdateByScan go on working in the window's frame: a world point p lies
        /// at p - Origin * Maps[0].CellLength there.  Not possible while ReferenceCache is on.</summary>
        public void Shift(int dx, int dy)
        {
            Native.Check(Native.slamhip_hs_shift(Pyramid.Ptr, dx, dy));
            MarkStale();
        }

        /// <summary>The pose-lattice search (slamhip_hs_lattice_search; the reference has no counterpart): the scan scored against the
        /// occupancy grid of level lattice.Level at every node of the lattice, whose centre is a pose in the window's frame.  Returns
        /// one key per heading -- ((uint)score ^ 0x80000000) &lt;&lt; 32 | (0xFFFFFFFF - flat): the best node of that heading -- and, when
        /// asked for, the whole score volume [k][iy][ix].  Blocking, behind everything already enqueued.</summary>
        public unsafe ulong[] LatticeSearch(ScanCloud scan, LatticeSpec lattice, bool wantScores, out int[] scores)
        {
            SetScan(scan);
            var keys = new ulong[Math.Max(0, lattice.NTheta)];
            scores = wantScores ? new int[(long)Math.Max(0, lattice.NTheta) * (2 * lattice.Ny + 1) * (2 * lattice.Nx + 1)] : null;
            fixed (ulong* k = keys)
            fixed (int* s = scores)
                Native.Check(Native.slamhip_hs_lattice_search(Pyramid.Ptr, lattice, k, s));
            return keys;
        }

        /// <summary>LatticeSearch over the world (slamhip_hs_world_lattice_search): a node's cell outside the window is the cell of the
        /// backing store's tile that holds it -- LogOddsCell.Reset() where none does -- so the lattice reaches everywhere the window has
        /// been.  The centre stays a pose in the window's frame.  With backing off the results are LatticeSearch's.</summary>
        public unsafe ulong[] WorldLatticeSearch(ScanCloud scan, LatticeSpec lattice, bool wantScores, out int[] scores)
        {
            SetScan(scan);
            var keys = new ulong[Math.Max(0, lattice.NTheta)];
            scores = wantScores ? new int[(long)Math.Max(0, lattice.NTheta) * (2 * lattice.Ny + 1) * (2 * lattice.Nx + 1)] : null;
            fixed (ulong* k = keys)
            fixed (int* s = scores)
                Native.Check(Native.slamhip_hs_world_lattice_search(Pyramid.Ptr, lattice, k, s));
            return keys;
        }

        /// <summary>The pose of node (k, flat) of that lattice in the window's frame (slamhip_hs_lattice_node_pose).</summary>
        public Vector3 LatticeNodePose(LatticeSpec lattice, int k, int flat)
        {
            Native.Check(Native.slamhip_hs_lattice_node_pose(Pyramid.Ptr, lattice, k, flat, out Vector3 pose));
            return pose;
        }

        /// <summary>The search's point cells for one heading, on the host (slamhip_debug_lattice_cells): (gx, gy) per point,
        /// int.MinValue twice for a point the search ignores.</summary>
        public static unsafe int[] LatticeCells(float cellLength, Vector3 centre, float theta, Vector2[] points)
        {
            var cells = new int[2 * points.Length];
            fixed (Vector2* p = points)
            fixed (int* c = cells)
                Native.Check(Native.slamhip_debug_lattice_cells(cellLength, centre, theta, p, points.Length, c));
            return cells;
        }

        /// <summary>The beam trace (slamhip_hs_trace; the reference has no counterpart): what the map of `level` holds along every
        /// beam of the scan from each of the poses (window frame) -- the grid update's own line from the sensor cell to the beam's end
        /// cell.  Returns one summary per pose and, when asked for, the beam records [pose][beam] (poses x beams at most 2^20).
        /// world: a cell outside the window is the cell of the backing store's tile that holds it.  Blocking; it changes nothing.</summary>
        public unsafe TraceSummary[] Trace(ScanCloud scan, Vector3[] poses, int level, bool world, bool wantBeams, out TraceBeam[] beams)
        {
            SetScan(scan);
            var sums = new TraceSummary[poses.Length];
            beams = wantBeams ? new TraceBeam[(long)poses.Length * scan.Points.Count] : null;
            fixed (Vector3* p = poses)
            fixed (TraceSummary* s = sums)
            fixed (TraceBeam* b = beams)
                Native.Check(Native.slamhip_hs_trace(Pyramid.Ptr, level, p, poses.Length, world ? 1 : 0, s, b));
            return sums;
        }

        /// <summary>The trace's lines on the host (slamhip_debug_trace_lines): {bx, by, ex, ey, da} per point for one pose on a level
        /// whose ScaleToMap is scaleToMap; an ignored beam is {0, 0, 0, 0, -1}.</summary>
        public static unsafe int[] TraceLines(float scaleToMap, Vector3 pose, Vector2 scanOrigin, Vector2[] points)
        {
            var lines = new int[5 * points.Length];
            fixed (Vector2* p = points)
            fixed (int* l = lines)
                Native.Check(Native.slamhip_debug_trace_lines(scaleToMap, pose, scanOrigin, p, points.Length, l));
            return lines;
        }

        /// <summary>The cells the trace walks from cell (bx, by) to cell (ex, ey), in order, x and y interleaved (slamhip_debug_trace_cells).</summary>
        public static unsafe int[] TraceCells(int bx, int by, int ex, int ey)
        {
            var cells = new int[2 * (Math.Min(Math.Max(Math.Abs((long)ex - bx), Math.Abs((long)ey - by)), 32768) + 1)];
            int n;
            fixed (int* c = cells)
                Native.Check(Native.slamhip_debug_trace_cells(bx, by, ex, ey, c, cells.Length / 2, out n));
            Array.Resize(ref cells, 2 * n);
            return cells;
        }

        /// <summary>The distance field (slamhip_hs_distance_field; the reference has no counterpart): for every cell of the rectangle
        /// (x, y, w, h), window-frame cells of `level`, the squared cell distance to the nearest site, capped at radius^2; [row * w +
        /// column].  A site is a cell whose class siteMask selects: bit 0 unknown, bit 1 occupied, bit 2 free (2: distance to
        /// obstacles).  radius in [1, 255].  world: a cell outside the window is the cell of the backing store's tile that holds it.
        /// Blocking; it changes nothing.</summary>
        public unsafe ushort[] DistanceField(int level, int x, int y, int w, int h, int siteMask = 2, int radius = 32, bool world = false)
        {
            var d2 = new ushort[(long)Math.Max(w, 0) * Math.Max(h, 0)];
            fixed (ushort* d = d2)
                Native.Check(Native.slamhip_hs_distance_field(Pyramid.Ptr, level, world ? 1 : 0, siteMask, radius, x, y, w, h, d));
            return d2;
        }

        /// <summary>The end-point distance score (slamhip_hs_distance_score): the field's value at the end cell of every point of
        /// `scan` at each of the poses (window frame).  Returns one summary per pose and, when asked for, the values [pose][point]
        /// (0xFFFF for an ignored point; poses x points at most 2^22).</summary>
        public unsafe DistanceSummary[] DistanceScore(ScanCloud scan, Vector3[] poses, int level, int siteMask, int radius, bool world, bool wantPoints, out ushort[] points)
        {
            SetScan(scan);
            var sums = new DistanceSummary[poses.Length];
            points = wantPoints ? new ushort[(long)poses.Length * scan.Points.Count] : null;
            fixed (Vector3* p = poses)
            fixed (DistanceSummary* s = sums)
            fixed (ushort* q = points)
                Native.Check(Native.slamhip_hs_distance_score(Pyramid.Ptr, level, world ? 1 : 0, siteMask, radius, p, poses.Length, s, q));
            return sums;
        }

        /// <summary>NearestField / NearestPairs: both components of a pair where no site lies within the radius, and of the
        /// per-point record of an ignored point.</summary>
        public const short NearestNone = short.MaxValue, NearestIgnored = short.MinValue;

        /// <summary>The nearest-site field (slamhip_hs_nearest_field; the reference has no counterpart): for every cell of the
        /// rectangle (x, y, w, h), window-frame cells of `level`, the offset (dx, dy) to the nearest site with dx^2 + dy^2 below
        /// radius^2 -- ties to the smaller row, then the smaller column -- as [2 * (row * w + column)] and the element behind it;
        /// NearestNone twice where there is none.  siteMask, radius and world as DistanceField.  Blocking; it changes nothing.</summary>
        public unsafe short[] NearestField(int level, int x, int y, int w, int h, int siteMask = 2, int radius = 32, bool world = false)
        {
            var dxdy = new short[2 * (long)Math.Max(w, 0) * Math.Max(h, 0)];
            fixed (short* d = dxdy)
                Native.Check(Native.slamhip_hs_nearest_field(Pyramid.Ptr, level, world ? 1 : 0, siteMask, radius, x, y, w, h, d));
            return dxdy;
        }

        /// <summary>The scan-to-map pairs (slamhip_hs_nearest_pairs): the nearest site of the end cell of every point of `scan` at
        /// each of the poses (window frame).  Returns one summary per pose and, when asked for, the offsets [2 * (pose * points +
        /// point)] (NearestIgnored twice for an ignored point, NearestNone twice for one without a site within the radius; poses x
        /// points at most 2^22).</summary>
        public unsafe PairSummary[] NearestPairs(ScanCloud scan, Vector3[] poses, int level, int siteMask, int radius, bool world, bool wantPairs, out short[] pairs)
        {
            SetScan(scan);
            var sums = new PairSummary[poses.Length];
            pairs = wantPairs ? new short[2 * (long)poses.Length * scan.Points.Count] : null;
            fixed (Vector3* p = poses)
            fixed (PairSummary* s = sums)
            fixed (short* q = pairs)
                Native.Check(Native.slamhip_hs_nearest_pairs(Pyramid.Ptr, level, world ? 1 : 0, siteMask, radius, p, poses.Length, s, q));
            return sums;
        }

        /// <summary>The nearest-site field of the definition over a caller's class array on the host (slamhip_debug_nearest_field):
        /// cls is ch rows of cw class bytes (1 occupied, 2 free, 0 neither), class 0 outside.</summary>
        public static unsafe short[] NearestFieldOf(byte[] cls, int cw, int ch, int siteMask, int radius, int x, int y, int w, int h)
        {
            var dxdy = new short[2 * (long)Math.Max(w, 0) * Math.Max(h, 0)];
            fixed (byte* c = cls)
            fixed (short* d = dxdy)
                Native.Check(Native.slamhip_debug_nearest_field(c, cw, ch, siteMask, radius, x, y, w, h, d));
            return dxdy;
        }

        /// <summary>One closed-form 2-D alignment step from ONE summary, host arithmetic only: the rigid motion e' = R(dTheta) e + t,
        /// in cells, that best takes the matched end cells onto their nearest sites, composed onto `pose` (the frame the summary
        /// was formed in) through the end cell's own transform e = stm (R(theta) p + T): theta' = theta + dTheta, T' = R(dTheta) T +
        /// t / stm.  The centred sums n S_ab - S_a S_b are formed exactly (BigInteger), then everything is double, rounded to
        /// float once.  basePose: the same pose in another frame of the same heading (a processor's world pose): the change T' - T
        /// is added to it, so a zero step hands it back bit for bit.  MatchedCount 1: a shift alone; 0: the pose as it is.</summary>
        public static Vector3 AlignStep(Vector3 pose, in PairSummary s, float stm, Vector3? basePose = null)
        {
            Vector3 b = basePose ?? pose;
            long n = s.MatchedCount;
            if (n < 1) return b;
            double dTheta = 0.0;
            if (n >= 2)
            {
                BigInteger N = n;
                var cross = (N * s.SumExQy - (BigInteger)s.SumEx * s.SumQy) - (N * s.SumEyQx - (BigInteger)s.SumEy * s.SumQx);
                var dot = (N * s.SumExQx - (BigInteger)s.SumEx * s.SumQx) + (N * s.SumEyQy - (BigInteger)s.SumEy * s.SumQy);
                dTheta = Math.Atan2((double)cross / n, (double)dot / n);
            }
            double c = Math.Cos(dTheta), sn = Math.Sin(dTheta);
            double tx = (s.SumQx - (c * s.SumEx - sn * s.SumEy)) / n;      // mean(q) - R mean(e), divided once: a pure shift comes out exact
            double ty = (s.SumQy - (sn * s.SumEx + c * s.SumEy)) / n;
            double x = pose.X, y = pose.Y, k = stm;
            return new Vector3((float)(b.X + ((c - 1.0) * x - sn * y + tx / k)), (float)(b.Y + (sn * x + (c - 1.0) * y + ty / k)), (float)(b.Z + dTheta));
        }

        /// <summary>The field of the definition over a caller's class array on the host (slamhip_debug_distance_field): cls is ch rows
        /// of cw class bytes (1 occupied, 2 free, 0 neither), class 0 outside.</summary>
        public static unsafe ushort[] DistanceFieldOf(byte[] cls, int cw, int ch, int siteMask, int radius, int x, int y, int w, int h)
        {
            var d2 = new ushort[(long)Math.Max(w, 0) * Math.Max(h, 0)];
            fixed (byte* c = cls)
            fixed (ushort* d = d2)
                Native.Check(Native.slamhip_debug_distance_field(c, cw, ch, siteMask, radius, x, y, w, h, d));
            return d2;
        }

        /// <summary>The frontier clusters of `level` (slamhip_hs_frontiers; the reference has no counterpart): the free cells that touch
        /// the unknown, grouped under 8-connectivity.  Returns the kept clusters (cells >= minCells), largest first, at most
        /// maxClusters, in window-frame cells of the level.  labelRect = (x, y, w, h), any position: labels receives [row * w + column]
        /// the label of every cell -- the flat index of its cluster's seed in the summary's map rectangle, -1 where the cell is no
        /// frontier cell; null: no labels.  Blocking; it changes nothing.</summary>
        public unsafe FrontierCluster[] Frontiers(int level, out FrontierSummary summary, int minCells = 1, int maxClusters = 256, bool world = false)
        {
            return Frontiers(level, out summary, minCells, maxClusters, world, null, out _);
        }

        public unsafe FrontierCluster[] Frontiers(int level, out FrontierSummary summary, int minCells, int maxClusters, bool world,
                                                  (int X, int Y, int W, int H)? labelRect, out int[] labels)
        {
            var rec = new FrontierCluster[Math.Max(maxClusters, 0)];
            var r = labelRect ?? (0, 0, 0, 0);
            labels = labelRect.HasValue ? new int[(long)Math.Max(r.W, 0) * Math.Max(r.H, 0)] : null;
            fixed (FrontierCluster* c = rec)
            fixed (int* l = labels)
                Native.Check(Native.slamhip_hs_frontiers(Pyramid.Ptr, level, world ? 1 : 0, minCells, maxClusters, out summary, c, r.X, r.Y, r.W, r.H, labelRect.HasValue ? l : null));
            Array.Resize(ref rec, summary.ReturnedCount);
            return rec;
        }

        /// <summary>The clusters of the definition over a caller's class array on the host (slamhip_debug_frontiers): cls is ch rows of
        /// cw class bytes (1 occupied, 2 free, 0 neither), class 0 outside; labels the whole cw x ch array.</summary>
        public static unsafe FrontierCluster[] FrontiersOf(byte[] cls, int cw, int ch, int minCells, int maxClusters, out FrontierSummary summary, out int[] labels)
        {
            var rec = new FrontierCluster[Math.Max(maxClusters, 0)];
            labels = new int[(long)Math.Max(cw, 0) * Math.Max(ch, 0)];
            fixed (byte* b = cls)
            fixed (FrontierCluster* c = rec)
            fixed (int* l = labels)
                Native.Check(Native.slamhip_debug_frontiers(b, cw, ch, minCells, maxClusters, out summary, c, l));
            Array.Resize(ref rec, summary.ReturnedCount);
            return rec;
        }

        /// <summary>The cost-to-go field of `spec.Level` (slamhip_hs_nav_field; the reference has no counterpart): the least 5-7 chamfer
        /// cost from the sources (x, y pairs, window-frame cells) to every traversable cell over moves that cut no corner.  goals: one
        /// rectangle {xMin, yMin, xMax, yMax} each, e.g. a frontier cluster's box grown as the caller sees fit; returns one result per
        /// goal.  The first nPaths goals get their cell path: paths[i] holds min(length, maxPathCells) (x, y) pairs, heads[i] the true
        /// length.  rect = (x, y, w, h), any position: cost and dir receive [row * w + column]; null: neither.  Blocking; it changes
        /// nothing.</summary>
        public unsafe NavGoalResult[] NavField(NavSpec spec, int[] sources, int[] goals, out NavSummary summary, int nPaths, int maxPathCells,
                                               out NavPath[] heads, out int[][] paths, (int X, int Y, int W, int H)? rect, out uint[] cost, out byte[] dir)
        {
            int nGoals = goals == null ? 0 : goals.Length / 4;
            var res = new NavGoalResult[nGoals];
            heads = new NavPath[Math.Max(nPaths, 0)];
            var cells = new int[2L * Math.Max(nPaths, 0) * Math.Max(maxPathCells, 0)];
            var r = rect ?? (0, 0, 0, 0);
            cost = rect.HasValue ? new uint[(long)Math.Max(r.W, 0) * Math.Max(r.H, 0)] : null;
            dir = rect.HasValue ? new byte[(long)Math.Max(r.W, 0) * Math.Max(r.H, 0)] : null;
            fixed (int* s = sources)
            fixed (int* g = goals)
            fixed (NavGoalResult* gr = res)
            fixed (NavPath* h = heads)
            fixed (int* pc = cells)
            fixed (uint* c = cost)
            fixed (byte* d = dir)
                Native.Check(Native.slamhip_hs_nav_field(Pyramid.Ptr, ref spec, s, sources.Length / 2, g, nGoals, gr, nPaths, maxPathCells, h, pc, r.X, r.Y, r.W, r.H, c, d, out summary));
            paths = NavPaths(heads, cells, maxPathCells);
            return res;
        }

        internal static int[][] NavPaths(NavPath[] heads, int[] cells, int maxPathCells)
        {
            var paths = new int[heads.Length][];
            for (int i = 0; i < heads.Length; i++)
            {
                paths[i] = new int[2 * heads[i].WrittenCount];
                Array.Copy(cells, 2L * i * maxPathCells, paths[i], 0, paths[i].Length);
            }
            return paths;
        }

        /// <summary>The field of the definition over a caller's class array on the host (slamhip_debug_nav_field): cls is ch rows of cw
        /// class bytes (1 occupied, 2 free, 0 neither), class 0 outside; cost and dir the whole cw x ch array; the costs come from a
        /// sequential Dijkstra.</summary>
        public static unsafe NavGoalResult[] NavFieldOf(byte[] cls, int cw, int ch, int siteMask, int clearance, uint maxCost, int[] sources, int[] goals,
                                                        out NavSummary summary, out uint[] cost, out byte[] dir)
        {
            int nGoals = goals == null ? 0 : goals.Length / 4;
            var res = new NavGoalResult[nGoals];
            cost = new uint[(long)Math.Max(cw, 0) * Math.Max(ch, 0)];
            dir = new byte[cost.Length];
            fixed (byte* b = cls)
            fixed (int* s = sources)
            fixed (int* g = goals)
            fixed (NavGoalResult* gr = res)
            fixed (uint* c = cost)
            fixed (byte* d = dir)
                Native.Check(Native.slamhip_debug_nav_field(b, cw, ch, siteMask, clearance, maxCost, s, sources.Length / 2, g, nGoals, gr, 0, 1, null, null, 0, 0, cw, ch, c, d, out summary));
            return res;
        }

        /// <summary>Command rollouts over the cost-to-go field of `spec.Level` (slamhip_hs_rollouts; the reference has no counterpart):
        /// each of the cmds.Length / (2 * nCmd) sequences of nCmd pairs (v, w), each pair held for `hold` steps of dt, is rolled
        /// forward from startPose (window frame) and cut at the first pose whose centre cell the field of `sources` does not reach or
        /// one of whose body points (pairs of metres in the robot's frame; null: none) lies on an untraversable cell.  Blocking; it
        /// changes nothing.</summary>
        public unsafe RolloutResult[] Rollouts(NavSpec spec, int[] sources, Vector3 startPose, float dt, float[] body, float[] cmds, int nCmd, int hold,
                                               out RolloutSummary summary)
        {
            int n = nCmd > 0 ? cmds.Length / (2 * nCmd) : 0;
            var res = new RolloutResult[Math.Max(n, 0)];
            var start = stackalloc float[3] { startPose.X, startPose.Y, startPose.Z };
            fixed (int* s = sources)
            fixed (float* b = body)
            fixed (float* c = cmds)
            fixed (RolloutResult* r = res)
                Native.Check(Native.slamhip_hs_rollouts(Pyramid.Ptr, ref spec, s, sources.Length / 2, start, dt, b, body == null ? 0 : body.Length / 2, c, n, nCmd, hold, r, out summary));
            return res;
        }

        /// <summary>The rollouts of the definition over a caller's class array on the host (slamhip_debug_rollouts): cls as for
        /// NavFieldOf, stm = 1 / cell length.</summary>
        public static unsafe RolloutResult[] RolloutsOf(byte[] cls, int cw, int ch, int siteMask, int clearance, uint maxCost, int[] sources, float stm, Vector3 startPose,
                                                        float dt, float[] body, float[] cmds, int nCmd, int hold, out RolloutSummary summary)
        {
            int n = nCmd > 0 ? cmds.Length / (2 * nCmd) : 0;
            var res = new RolloutResult[Math.Max(n, 0)];
            var start = stackalloc float[3] { startPose.X, startPose.Y, startPose.Z };
            fixed (byte* k = cls)
            fixed (int* s = sources)
            fixed (float* b = body)
            fixed (float* c = cmds)
            fixed (RolloutResult* r = res)
                Native.Check(Native.slamhip_debug_rollouts(k, cw, ch, siteMask, clearance, maxCost, s, sources.Length / 2, stm, start, dt, b, body == null ? 0 : body.Length / 2,
                                                           c, n, nCmd, hold, r, out summary));
            return res;
        }

        /// <summary>The particle set of the localisation filter (slamhip_hs_mcl_set): poses in the window's frame, at most 65536; every
        /// accumulated cost becomes 0.  It replaces any previous set.</summary>
        public unsafe void MclSet(Vector3[] poses)
        {
            fixed (Vector3* p = poses)
                Native.Check(Native.slamhip_hs_mcl_set(Pyramid.Ptr, p, poses.Length));
            mclCount = poses.Length;
        }
        private int mclCount;

        /// <summary>One localisation step on the particle set against the scan that was set (slamhip_hs_mcl_step; the reference has no
        /// counterpart): predict by odometry with noise, weigh against the distance field, resample -- all on the device.  Blocking;
        /// it changes nothing of the map.</summary>
        public MclSummary MclStep(in MclSpec spec)
        {
            Native.Check(Native.slamhip_hs_mcl_step(Pyramid.Ptr, spec, out MclSummary summary));
            return summary;
        }

        /// <summary>The particle set as it stands (slamhip_hs_mcl_get): poses, accumulated costs, the ancestors of the last step.</summary>
        public unsafe Vector3[] MclGet(out ulong[] acc, out int[] ancestors)
        {
            var poses = new Vector3[mclCount];
            acc = new ulong[mclCount]; ancestors = new int[mclCount];
            fixed (Vector3* p = poses)
            fixed (ulong* a = acc)
            fixed (int* k = ancestors)
                Native.Check(Native.slamhip_hs_mcl_get(Pyramid.Ptr, p, a, k, mclCount));
            return poses;
        }

        /// <summary>One localisation step of the definition over a caller's class array on the host (slamhip_debug_mcl_step): cls as for
        /// NavFieldOf, stm = 1 / cell length, accIn null for zeros.</summary>
        public static unsafe Vector3[] MclStepOf(byte[] cls, int cw, int ch, float stm, Vector2[] points, Vector3[] particles, ulong[] accIn, in MclSpec spec,
                                                 out ulong[] acc, out int[] ancestors, out MclSummary summary)
        {
            var res = new Vector3[particles.Length];
            acc = new ulong[particles.Length]; ancestors = new int[particles.Length];
            fixed (byte* c = cls)
            fixed (Vector2* q = points)
            fixed (Vector3* p = particles)
            fixed (ulong* ai = accIn)
            fixed (Vector3* r = res)
            fixed (ulong* a = acc)
            fixed (int* k = ancestors)
                Native.Check(Native.slamhip_debug_mcl_step(c, cw, ch, stm, q, points.Length, p, ai, particles.Length, spec, r, a, k, out summary));
            return res;
        }

        /// <summary>The source map of the merge (slamhip_hs_merge_set_source; the reference has no counterpart): cells, row-major w x h,
        /// the first source-frame cell (ax, ay) of a grid with the level's cell length -- what DownloadCells or WorldCells of any pyramid
        /// gives.  It stays in device memory until the next MergeSetSource, MergeClearSource or Reset.</summary>
        public unsafe void MergeSetSource(int level, int ax, int ay, int w, int h, LogOddsCell[] cells)
        {
            if (cells.Length != w * h) throw new ArgumentException("cells must hold w * h elements");
            fixed (LogOddsCell* c = cells)
                Native.Check(Native.slamhip_hs_merge_set_source(Pyramid.Ptr, level, ax, ay, w, h, c));
        }

        /// <summary>Rate candidate alignments of the source with its level (slamhip_hs_merge_score): each pose the origin and heading of
        /// the SOURCE frame in the window's frame, at most 4096.  Blocking; it changes nothing.</summary>
        public unsafe MergeReport[] MergeScore(Vector3[] poses)
        {
            var reports = new MergeReport[poses.Length];
            fixed (Vector3* p = poses)
            fixed (MergeReport* r = reports)
                Native.Check(Native.slamhip_hs_merge_score(Pyramid.Ptr, p, poses.Length, r));
            return reports;
        }

        /// <summary>Fuse the source into its level at one pose on the device (slamhip_hs_merge_apply): rule 0 add (cut to +-valueLimit),
        /// 1 fill unknown cells, 2 replace.  Blocking.</summary>
        public MergeReport MergeApply(Vector3 pose, int rule, float valueLimit)
        {
            Native.Check(Native.slamhip_hs_merge_apply(Pyramid.Ptr, pose, rule, valueLimit, out MergeReport report));
            return report;
        }

        /// <summary>No source from here on (slamhip_hs_merge_clear_source).</summary>
        public void MergeClearSource() => Native.Check(Native.slamhip_hs_merge_clear_source(Pyramid.Ptr));

        /// <summary>The Hough transform of a map into a slot (slamhip_hs_hough; the reference has no counterpart): slot 0 the map of
        /// `level` (the window's, or the world rectangle's), slot 1 the merge source (level must be its level, world false).  nAngles a
        /// multiple of 4 in [4, 1024], bins of 2^q cells.  Blocking; it changes nothing of the map.</summary>
        public HoughInfo Hough(int level, int slot = 0, bool world = false, int siteMask = 2, int nAngles = 360, int q = 1, bool wantVotes = false)
            => HoughCall(false, Pyramid.Ptr, level, slot, world, siteMask, nAngles, q, wantVotes);

        internal readonly HoughInfo[] HoughSlots = new HoughInfo[2];       // what the last Hough call of each slot reported

        internal unsafe HoughInfo HoughCall(bool throughProcessor, IntPtr handle, int level, int slot, bool world, int siteMask, int nAngles, int q, bool wantVotes)
        {
            var info = stackalloc int[7];
            var r = new HoughInfo { T = nAngles, Q = q, Spectrum = new ulong[Math.Max(nAngles, 0)] };
            uint[] votes = wantVotes ? new uint[1 << 24] : null;           // (N is the call's own result: room for the most the limits allow)
            fixed (ulong* s = r.Spectrum)
            fixed (uint* v = votes)
                Native.Check(throughProcessor ? Native.slamhip_hsproc_hough(handle, level, slot, world ? 1 : 0, siteMask, nAngles, q, info, s, v)
                                              : Native.slamhip_hs_hough(handle, level, slot, world ? 1 : 0, siteMask, nAngles, q, info, s, v));
            r.W = info[0]; r.H = info[1]; r.X0 = info[2]; r.Y0 = info[3]; r.D = info[4]; r.N = info[5]; r.Sites = info[6];
            if (wantVotes) { r.Votes = new uint[(long)nAngles * r.N]; Array.Copy(votes, r.Votes, r.Votes.Length); }
            if (slot == 0 || slot == 1) HoughSlots[slot] = r;
            return r;
        }

        /// <summary>The rotation scores CC of the two filled slots (slamhip_hs_hough_rotation): CC peaks where the source frame is
        /// turned by m pi / T (mod pi) in the destination's frame.</summary>
        public unsafe ulong[] HoughRotation()
        {
            if (HoughSlots[0] == null) throw new InvalidOperationException("fill both slots (Hough) first");
            var cc = new ulong[HoughSlots[0].T];
            fixed (ulong* c = cc)
                Native.Check(Native.slamhip_hs_hough_rotation(Pyramid.Ptr, c));
            return cc;
        }

        /// <summary>The row correlations of pairs (m, k), flattened (slamhip_hs_hough_shifts), at most 256 pairs.</summary>
        public unsafe HoughShift[] HoughShifts(int[] pairs)
        {
            var res = new HoughShift[pairs.Length / 2];
            fixed (int* p = pairs)
            fixed (HoughShift* r = res)
                Native.Check(Native.slamhip_hs_hough_shifts(Pyramid.Ptr, p, res.Length, r, null));
            return res;
        }

        internal int SigRings;                                             // n_ring of the last SigConfigure: sizes the word arrays

        /// <summary>Set the spec of the scan signatures and EMPTY the keyframe store (slamhip_hs_sig_configure; the reference has no
        /// counterpart): ringCount rings of ringCells cells each, 64 sectors, `scale` cells per metre.</summary>
        public void SigConfigure(float scale, int ringCount, int ringCells)
        {
            var spec = new SigSpec { Scale = scale, RingCount = ringCount, RingCells = ringCells };
            Native.Check(Native.slamhip_hs_sig_configure(Pyramid.Ptr, spec));
            SigRings = ringCount;
        }

        /// <summary>The signature of the scan SetScan took, appended to the store with `pose` (opaque to the library;
        /// slamhip_hs_sig_add).  Returns the new keyframe's index.</summary>
        public unsafe int SigAdd(Vector3 pose, out ulong[] signature, out SigInfo info)
        {
            signature = new ulong[SigRings];
            int index;
            fixed (ulong* s = signature)
                Native.Check(Native.slamhip_hs_sig_add(Pyramid.Ptr, pose, out index, s, out info));
            return index;
        }

        /// <summary>Many scans of a log appended in ONE launch (slamhip_hs_sig_add_scans): scan b is points[offsets[b] .. offsets[b + 1]).
        /// Returns the first new index.</summary>
        public unsafe int SigAddScans(Vector2[] points, int[] offsets, Vector3[] poses)
        {
            int first;
            fixed (Vector2* p = points)
            fixed (int* o = offsets)
            fixed (Vector3* q = poses)
                Native.Check(Native.slamhip_hs_sig_add_scans(Pyramid.Ptr, p, o, poses.Length, q, out first));
            return first;
        }

        public int SigCount
        {
            get { Native.Check(Native.slamhip_hs_sig_count(Pyramid.Ptr, out int n)); return n; }
        }

        /// <summary>The scan SetScan took against the keyframes [first, last) over all 64 headings (slamhip_hs_sig_query): at most
        /// maxHits (up to 16) hits, higher score first, then lower index.  Nothing is appended.</summary>
        public unsafe SigHit[] SigQuery(int first, int last, int maxHits)
        {
            var hits = new SigHit[16];
            int n;
            fixed (SigHit* h = hits)
                Native.Check(Native.slamhip_hs_sig_query(Pyramid.Ptr, first, last, maxHits, h, out n, null, out _));
            Array.Resize(ref hits, n);
            return hits;
        }

        /// <summary>Every keyframe i of [first, last) against the keyframes [first, i - minGap] (slamhip_hs_sig_self): one hit per
        /// keyframe, Index -1 where that range is empty.</summary>
        public unsafe SigHit[] SigSelf(int first, int last, int minGap)
        {
            var hits = new SigHit[Math.Max(last - first, 1)];
            fixed (SigHit* h = hits)
                Native.Check(Native.slamhip_hs_sig_self(Pyramid.Ptr, first, last, minGap, h));
            Array.Resize(ref hits, Math.Max(last - first, 0));
            return hits;
        }

        /// <summary>Keyframes [first, first + n) out of the store, key-major words and poses (slamhip_hs_sig_download).</summary>
        public unsafe void SigDownload(int first, int n, out ulong[] signatures, out Vector3[] poses)
        {
            signatures = new ulong[Math.Max(n, 0) * SigRings + 1]; poses = new Vector3[Math.Max(n, 0) + 1];
            fixed (ulong* s = signatures)
            fixed (Vector3* p = poses)
                Native.Check(Native.slamhip_hs_sig_download(Pyramid.Ptr, first, n, s, p));
            Array.Resize(ref signatures, Math.Max(n, 0) * SigRings); Array.Resize(ref poses, Math.Max(n, 0));
        }

        /// <summary>Keyframes appended from what SigDownload gave (slamhip_hs_sig_upload); the library counts the bits itself.</summary>
        public unsafe void SigUpload(ulong[] signatures, Vector3[] poses)
        {
            fixed (ulong* s = signatures)
            fixed (Vector3* p = poses)
                Native.Check(Native.slamhip_hs_sig_upload(Pyramid.Ptr, poses.Length, s, p));
        }

        /// <summary>Overwrite the stored poses of keyframes [first, first + poses.Length) (slamhip_hs_sig_set_poses; host-side, nothing
        /// is launched).</summary>
        public unsafe void SigSetPoses(int first, Vector3[] poses)
        {
            fixed (Vector3* p = poses)
                Native.Check(Native.slamhip_hs_sig_set_poses(Pyramid.Ptr, first, poses.Length, p));
        }

        /// <summary>Nodes and edges of the pose graph PgSet took.</summary>
        public int PgNodes { get; private set; }
        public int PgEdges { get; private set; }

        /// <summary>Take a pose graph, replacing any earlier one (slamhip_hs_pg_set): poses = N x 3 doubles (x, y, theta), isFixed a
        /// byte per node or null (node 0 alone), ij = E x 2, z and w = E x 3.</summary>
        public unsafe void PgSet(double[] poses, byte[] isFixed, int[] ij, double[] z, double[] w)
        {
            int n = poses.Length / 3, e = ij.Length / 2;
            fixed (double* pp = poses, pz = z, pw = w)
            fixed (byte* pf = isFixed)
            fixed (int* pe = ij)
                Native.Check(Native.slamhip_hs_pg_set(Pyramid.Ptr, pp, pf, n, pe, pz, pw, e));
            PgNodes = n; PgEdges = e;
        }

        /// <summary>spec.OuterCount Gauss-Newton steps from the poses as they stand (slamhip_hs_pg_relax).</summary>
        public unsafe PgIter[] PgRelax(PgSpec spec, out double chi2Final)
        {
            var iters = new PgIter[Math.Max(spec.OuterCount, 1)];
            fixed (PgIter* p = iters)
                Native.Check(Native.slamhip_hs_pg_relax(Pyramid.Ptr, in spec, p, out chi2Final));
            return iters;
        }

        /// <summary>PgRelax with the odometry-chain preconditioner when tri is true (slamhip_hs_pg_relax_tri: the block-tridiagonal part
        /// of H, the one for a chain of keyframes closed by a few loops); block-Jacobi otherwise.</summary>
        public unsafe PgIter[] PgRelax(PgSpec spec, bool tri, out double chi2Final)
        {
            if (!tri) return PgRelax(spec, out chi2Final);
            var iters = new PgIter[Math.Max(spec.OuterCount, 1)];
            fixed (PgIter* p = iters)
                Native.Check(Native.slamhip_hs_pg_relax_tri(Pyramid.Ptr, in spec, p, out chi2Final));
            return iters;
        }

        /// <summary>Damped and robust relaxation from the poses as they stand (slamhip_hs_pg_relax_lm, rules R1 - R4): robust, a byte per
        /// edge or null for every edge, says which edges the spec's kernel applies to.  Returns one record per attempt made; factors,
        /// if given (PgEdges entries), receives every edge's factor at the final poses.</summary>
        public unsafe PgLmIter[] PgRelaxLm(PgLmSpec spec, byte[] robust, out double costFinal, double[] factors = null)
        {
            if (robust != null && robust.Length != PgEdges) throw new ArgumentException("robust: one byte per edge");
            if (factors != null && factors.Length != PgEdges) throw new ArgumentException("factors: one entry per edge");
            var iters = new PgLmIter[Math.Max(spec.OuterCount, 1)];
            int count;
            fixed (PgLmIter* p = iters)
            fixed (byte* r = robust)
            fixed (double* f = factors)
                Native.Check(Native.slamhip_hs_pg_relax_lm(Pyramid.Ptr, in spec, r, p, out count, out costFinal, f));
            Array.Resize(ref iters, count);
            return iters;
        }

        /// <summary>Marginal covariances at the poses as they stand (slamhip_hs_pg_marginals, rules M1 - M5): pairs = P x 2 node indices
        /// (n, m); returns P x 9 doubles, block p = Sigma[n_p][m_p] row-major (+0 where n_p or m_p is fixed).  cols receives one record per
        /// right-hand side, info what was done.  Neither the poses nor a later relaxation's results change.</summary>
        public unsafe double[] PgMarginals(PgMargSpec spec, int[] pairs, out PgMargCol[] cols, out PgMargInfo info)
        {
            if (pairs == null || pairs.Length < 2 || (pairs.Length & 1) != 0) throw new ArgumentException("pairs: P x 2 node indices");
            int nPairs = pairs.Length / 2, count;
            var blocks = new double[9 * nPairs];
            cols = new PgMargCol[3 * Math.Min(nPairs, 4096)];
            fixed (int* pr = pairs)
            fixed (double* b = blocks)
            fixed (PgMargCol* c = cols)
                Native.Check(Native.slamhip_hs_pg_marginals(Pyramid.Ptr, in spec, pr, nPairs, b, c, out count, out info));
            Array.Resize(ref cols, count);
            return blocks;
        }

        /// <summary>z = T^-1 rhs at the poses as they stand (slamhip_hs_pg_tri_apply): N x 3 doubles in, N x 3 doubles out.</summary>
        public unsafe double[] PgTriApply(double lambda, double[] rhs)
        {
            if (rhs.Length != Math.Max(PgNodes, 1) * 3) throw new ArgumentException("rhs: N x 3 doubles");
            var z = new double[rhs.Length];
            fixed (double* r = rhs, o = z)
                Native.Check(Native.slamhip_hs_pg_tri_apply(Pyramid.Ptr, lambda, r, o));
            return z;
        }

        /// <summary>The graph's poses as they stand (slamhip_hs_pg_get): N x 3 doubles.</summary>
        public unsafe double[] PgGet()
        {
            var poses = new double[Math.Max(PgNodes, 1) * 3];
            fixed (double* p = poses)
                Native.Check(Native.slamhip_hs_pg_get(Pyramid.Ptr, p, PgNodes));
            return poses;
        }

        /// <summary>Residuals (E x 3) and chi2 per edge at the poses as they stand (slamhip_hs_pg_residuals).</summary>
        public unsafe void PgResiduals(out double[] r, out double[] chi2)
        {
            r = new double[Math.Max(PgEdges, 1) * 3]; chi2 = new double[Math.Max(PgEdges, 1)];
            fixed (double* pr = r, pc = chi2)
                Native.Check(Native.slamhip_hs_pg_residuals(Pyramid.Ptr, pr, pc));
            Array.Resize(ref r, PgEdges * 3); Array.Resize(ref chi2, PgEdges);
        }

        /// <summary>Free the blocks of the pose graph (slamhip_hs_pg_clear).</summary>
        public void PgClear()
        {
            Native.Check(Native.slamhip_hs_pg_clear(Pyramid.Ptr));
            PgNodes = PgEdges = 0;
        }

        /// <summary>Append a scan to the device-resident scan store (slamhip_hs_scans_add): null = the scan SetScan took.
        /// Returns its index; HectorSLAMProcessor keeps it equal to the keyframe's index in the signature store.</summary>
        public unsafe int ScansAdd(ScanCloud scan = null)
        {
            int index;
            if (scan == null) { Native.Check(Native.slamhip_hs_scans_add(Pyramid.Ptr, null, 0, null, out index)); return index; }
            Vector2[] pts = scan.Points.Count > 0 ? scan.Points.ToArray() : new Vector2[1];
            Vector2 origin = new Vector2(scan.Pose.X, scan.Pose.Y);
            fixed (Vector2* p = pts) Native.Check(Native.slamhip_hs_scans_add(Pyramid.Ptr, p, scan.Points.Count, &origin, out index));
            return index;
        }

        public int ScansCount
        {
            get { Native.Check(Native.slamhip_hs_scans_count(Pyramid.Ptr, out int n)); return n; }
        }

        /// <summary>Scan k of the store (slamhip_hs_scans_info, slamhip_hs_scans_download).</summary>
        public unsafe Vector2[] ScansGet(int k, out Vector2 scanOrigin)
        {
            Native.Check(Native.slamhip_hs_scans_info(Pyramid.Ptr, k, out int n, out scanOrigin));
            var pts = new Vector2[Math.Max(n, 1)];
            fixed (Vector2* p = pts) Native.Check(Native.slamhip_hs_scans_download(Pyramid.Ptr, k, p, n));
            Array.Resize(ref pts, n);
            return pts;
        }

        /// <summary>Free the scan store (slamhip_hs_scans_clear).</summary>
        public void ScansClear()
        {
            Native.Check(Native.slamhip_hs_scans_clear(Pyramid.Ptr));
        }

        /// <summary>Draw scans [first, last) of the scan store into the pyramid at the given window-frame poses, as that many SetScan +
        /// UpdateByScan calls in order would, in one call (slamhip_hs_render).  Without keep the map is cleared first.</summary>
        public unsafe void Render(Vector3[] poses, int first, int last, bool keep = false)
        {
            Vector3[] p = poses != null && poses.Length > 0 ? poses : new Vector3[1];
            fixed (Vector3* pp = p) Native.Check(Native.slamhip_hs_render(Pyramid.Ptr, first, last, pp, keep ? 1 : 0));
        }

        /// <summary>Match stored scans pairwise (slamhip_hs_scans_match): per pair the best node of the lattice round its guess, an
        /// integer score and the moments of the near-optimal nodes.</summary>
        public unsafe ScanMatchResult[] ScansMatch(ScanMatchSpec spec, ScanPair[] pairs)
        {
            var res = new ScanMatchResult[Math.Max(pairs.Length, 1)];
            ScanPair[] pr = pairs.Length > 0 ? pairs : new ScanPair[1];
            fixed (ScanPair* p = pr) fixed (ScanMatchResult* r = res)
                Native.Check(Native.slamhip_hs_scans_match(Pyramid.Ptr, spec, p, pairs.Length, r));
            Array.Resize(ref res, pairs.Length);
            return res;
        }

        /// <summary>The results of ScansMatch as pose-graph edges (slamhip_hs_scans_edges; host only): z and w hold three doubles
        /// per pair, valid one flag.</summary>
        public static unsafe void ScansEdges(ScanMatchSpec spec, ScanPair[] pairs, ScanMatchResult[] results, out double[] z, out double[] w, out bool[] valid)
        {
            int n = pairs.Length;
            z = new double[3 * Math.Max(n, 1)]; w = new double[3 * Math.Max(n, 1)];
            var v = new int[Math.Max(n, 1)];
            fixed (ScanPair* p = pairs) fixed (ScanMatchResult* r = results) fixed (double* pz = z, pw = w) fixed (int* pv = v)
                Native.Check(Native.slamhip_hs_scans_edges(spec, p, r, n, pz, pw, pv));
            valid = new bool[n];
            for (int i = 0; i < n; i++) valid[i] = v[i] != 0;
        }

        /// <summary>Rules 1 - 5 of slamhip_hs_scans_match on the host (slamhip_debug_scans_match; no device involved): points holds all
        /// scans one behind the other, offsets their starts and the total.</summary>
        public static unsafe ScanMatchResult[] DebugScansMatch(Vector2[] points, int[] offsets, ScanMatchSpec spec, ScanPair[] pairs)
        {
            var res = new ScanMatchResult[Math.Max(pairs.Length, 1)];
            Vector2[] pts = points.Length > 0 ? points : new Vector2[1];
            fixed (Vector2* xy = pts) fixed (int* off = offsets) fixed (ScanPair* p = pairs) fixed (ScanMatchResult* r = res)
                Native.Check(Native.slamhip_debug_scans_match(xy, off, offsets.Length - 1, spec, p, pairs.Length, r));
            Array.Resize(ref res, pairs.Length);
            return res;
        }

        /// <summary>Free the blocks of the scan signatures and forget the spec (slamhip_hs_sig_clear).</summary>
        public void SigClear()
        {
            Native.Check(Native.slamhip_hs_sig_clear(Pyramid.Ptr));
            SigRings = 0;
        }

        /// <summary>Free the blocks of the Hough transform (slamhip_hs_hough_clear); both slots are empty afterwards.</summary>
        public void HoughClear()
        {
            Native.Check(Native.slamhip_hs_hough_clear(Pyramid.Ptr));
            HoughSlots[0] = HoughSlots[1] = null;
        }

        /// <summary>The rotation hypotheses of AlignMaps from CC: the m with CC[m] > CC[m - 1] and CC[m] >= CC[m + 1], circularly,
        /// ranked by CC descending then m ascending; the best nRot, or {0} if there is none.</summary>
        public static int[] HoughPeaks(ulong[] cc, int nRot)
        {
            int T = cc.Length;
            var peaks = new System.Collections.Generic.List<int>();
            for (int m = 0; m < T; m++)
                if (cc[m] > cc[(m + T - 1) % T] && cc[m] >= cc[(m + 1) % T]) peaks.Add(m);
            peaks.Sort((a, b) => cc[a] != cc[b] ? cc[b].CompareTo(cc[a]) : a.CompareTo(b));
            if (peaks.Count > nRot) peaks.RemoveRange(nRot, peaks.Count - nRot);
            if (peaks.Count == 0) peaks.Add(0);
            return peaks.ToArray();
        }

        /// <summary>The pose (tx, ty, theta) of the source frame in the destination's from the shift records of pairs (m, ka) and
        /// (m, kb), by the formula of include/slamhip.h (slamhip_hs_hough): binary64 on the host, theta = m pi / T in (-pi, pi].</summary>
        public static Vector3 HoughPose(int m, HoughShift a, int ka, HoughShift b, int kb, HoughInfo d, HoughInfo s, float stm)
        {
            int T = d.T, bin = 1 << d.Q;
            double theta = m * Math.PI / T;
            var n = new double[2, 2]; var rhs = new double[2];
            for (int i = 0; i < 2; i++) {
                int k = i == 0 ? ka : kb, kk = k - m; bool f = false;
                while (kk < 0) { kk += T; f = !f; }
                double psi = k * Math.PI / T;
                n[i, 0] = Math.Cos(psi); n[i, 1] = Math.Sin(psi);
                rhs[i] = (double)bin * (i == 0 ? a : b).BestShift + d.X0 * n[i, 0] + d.Y0 * n[i, 1] - s.X0 * Math.Cos(psi - theta) - s.Y0 * Math.Sin(psi - theta)
                         - d.D + s.D + (f ? bin - 1 - (2 * s.D) % bin : 0);
            }
            double det = n[0, 0] * n[1, 1] - n[0, 1] * n[1, 0];
            double tx = (rhs[0] * n[1, 1] - rhs[1] * n[0, 1]) / det, ty = (n[0, 0] * rhs[1] - n[1, 0] * rhs[0]) / det;
            double th = Math.IEEERemainder(theta, 2.0 * Math.PI);
            if (th <= -Math.PI) th += 2.0 * Math.PI;
            return new Vector3((float)(tx / stm), (float)(ty / stm), (float)th);
        }

        /// <summary>The merge of the definition on the host (slamhip_debug_merge): no device involved.</summary>
        public static unsafe LogOddsCell[] MergeOf(LogOddsCell[] dst, int dw, int dh, LogOddsCell[] src, int ax, int ay, int sw, int sh, Vector3 pose, float stm, int rule,
                                                   float valueLimit, out MergeReport report)
        {
            var res = new LogOddsCell[dst.Length];
            fixed (LogOddsCell* d = dst)
            fixed (LogOddsCell* s = src)
            fixed (LogOddsCell* r = res)
                Native.Check(Native.slamhip_debug_merge(d, dw, dh, s, ax, ay, sw, sh, pose, stm, rule, valueLimit, r, out report));
            return res;
        }

        /// <summary>The kernels' tile box of a destination tile (slamhip_debug_merge_box): {u0, v0, u1, v1} in cells of the source array,
        /// or null when no cell of the tile is sourced.</summary>
        public static unsafe int[] MergeBoxOf(Vector3 pose, float stm, int ax, int ay, int sw, int sh, int x0, int y0, int x1, int y1)
        {
            var box = new int[4];
            int any;
            fixed (int* b = box) Native.Check(Native.slamhip_debug_merge_box(pose, stm, ax, ay, sw, sh, x0, y0, x1, y1, b, out any));
            return any != 0 ? box : null;
        }

        /// <summary>The view gain (slamhip_hs_view_gain; the reference has no counterpart): the DISTINCT cells of `level` the scan's beams
        /// see from each pose (window frame, at most 4096), no further than `reach` cells, by class and against the covered layer as it
        /// was before the call.  commit: -1 nothing, -2 every pose's cells join the layer, an index that pose's.  Blocking; it changes
        /// nothing of the map.</summary>
        public unsafe ViewSummary[] ViewGain(ScanCloud scan, Vector3[] poses, int level, int reach, int commit = -1)
        {
            SetScan(scan);
            var sums = new ViewSummary[poses.Length];
            fixed (Vector3* p = poses)
            fixed (ViewSummary* s = sums)
                Native.Check(Native.slamhip_hs_view_gain(Pyramid.Ptr, level, reach, p, poses.Length, commit, s));
            return sums;
        }

        /// <summary>The greedy choice of views (slamhip_hs_view_select): up to k of the poses, each round the one that adds the most new
        /// cells (mode 0) or new unknown cells (mode 1) to the covered layer, ties to the lowest index, until the best adds fewer than
        /// minGain.  Returns the chosen pose indices in the order of choice; gains their gains.  The chosen views join the layer.</summary>
        public unsafe int[] ViewSelect(ScanCloud scan, Vector3[] poses, int level, int reach, int k, int mode, int minGain, out int[] gains)
        {
            SetScan(scan);
            var order = new int[k];
            var gain = new int[k];
            int n;
            fixed (Vector3* p = poses)
            fixed (int* o = order)
            fixed (int* g = gain)
                Native.Check(Native.slamhip_hs_view_select(Pyramid.Ptr, level, reach, mode, minGain, p, poses.Length, k, o, g, out n));
            Array.Resize(ref order, n);
            Array.Resize(ref gain, n);
            gains = gain;
            return order;
        }

        /// <summary>Set the covered layer of `level` (slamhip_hs_view_set_covered): rows of (w + 31) / 32 words, cell x bit x &amp; 31 of word
        /// x >> 5; null: empty.</summary>
        public unsafe void SetCovered(int level, uint[] bits)
        {
            fixed (uint* b = bits) Native.Check(Native.slamhip_hs_view_set_covered(Pyramid.Ptr, level, b));
        }

        /// <summary>The covered layer of `level` (slamhip_hs_view_get_covered), in SetCovered's layout.</summary>
        public unsafe uint[] GetCovered(int level)
        {
            var dims = Maps[level].Dimensions;
            var bits = new uint[((dims.X + 31) / 32) * dims.Y];
            fixed (uint* b = bits) Native.Check(Native.slamhip_hs_view_get_covered(Pyramid.Ptr, level, b));
            return bits;
        }

        /// <summary>Free every block of the view gain, the covered layer too (slamhip_hs_view_clear).</summary>
        public void ViewClear() => Native.Check(Native.slamhip_hs_view_clear(Pyramid.Ptr));

        /// <summary>One pose's seen cells and summary on the host (slamhip_debug_view): no device involved.  values: w * h cell Values,
        /// row-major; covered: SetCovered's layout or null.</summary>
        public static unsafe uint[] ViewOf(float[] values, int w, int h, float scaleToMap, Vector3 pose, Vector2 scanOrigin, Vector2[] points, int reach, uint[] covered,
                                           out ViewSummary summary)
        {
            var bits = new uint[((w + 31) / 32) * h];
            fixed (float* v = values)
            fixed (Vector2* p = points)
            fixed (uint* c = covered)
            fixed (uint* b = bits)
                Native.Check(Native.slamhip_debug_view(v, w, h, scaleToMap, pose, scanOrigin, p, points.Length, reach, c, b, out summary));
            return bits;
        }

        /// <summary>The weight table of the localisation step (slamhip_debug_mcl_table).</summary>
        public static unsafe uint[] MclTable()
        {
            var t = new uint[64];
            fixed (uint* p = t) Native.Check(Native.slamhip_debug_mcl_table(p));
            return t;
        }

        /// <summary>The sum of all shifts since construction or the last Reset, in level-0 cells (slamhip_hs_origin).</summary>
        public (long X, long Y) Origin
        {
            get
            {
                Native.Check(Native.slamhip_hs_origin(Pyramid.Ptr, out long ox, out long oy));
                return (ox, oy);
            }
        }

        /// <summary>The backing store of the scrolling window (slamhip_hs_set_backing): with maxBytes > 0, what Shift moves out of the
        /// window is kept in a device pool of at most maxBytes, in world tiles of tileCells x tileCells cells per level (a power of two
        /// in [8, 256]), and restored when the window returns; a shift never fails for capacity -- pieces that find no slot are dropped
        /// and counted.  maxBytes = 0 (the default state): off, the pool is freed.  The setting survives Reset, the tiles do not.</summary>
        public void SetBacking(int tileCells, ulong maxBytes)
        {
            Native.Check(Native.slamhip_hs_set_backing(Pyramid.Ptr, tileCells, maxBytes));
        }

        /// <summary>slamhip_hs_backing_stats: all zero while backing is off.</summary>
        public BackingStats BackingStats
        {
            get
            {
                Native.Check(Native.slamhip_hs_backing_stats(Pyramid.Ptr, out BackingStats st));
                return st;
            }
        }

        /// <summary>The rectangle [x0, x0 + w) x [y0, y0 + h) of `level` in WORLD cells, row-major (slamhip_hs_world_cells_download): the
        /// window's cells from the window, evicted cells from their tiles, LogOddsCell.Reset() everywhere else.  Blocking; w * h at
        /// most 2^26.  Works with backing off: the window in a frame of Reset cells.</summary>
        public unsafe LogOddsCell[] WorldCells(int level, long x0, long y0, int w, int h)
        {
            var cells = new LogOddsCell[Math.Max(0, (long)w * h)];
            fixed (LogOddsCell* p = cells)
                Native.Check(Native.slamhip_hs_world_cells_download(Pyramid.Ptr, level, x0, y0, w, h, p));
            return cells;
        }

        /// <summary>The inverse of WorldCells (slamhip_hs_world_cells_upload): cells[w * h], row-major, replaces the rectangle
        /// [x0, x0 + w) x [y0, y0 + h) of `level` in WORLD cells -- the window's part in the window, the rest in tile slots when
        /// backing is on (a tile is made only where the rectangle holds a cell that is not LogOddsCell.Reset()).  Returns the
        /// non-Reset cells dropped: everything outside the window with backing off, what found no slot with backing on.  Blocking;
        /// never fails for capacity.</summary>
        public unsafe long WorldPut(int level, long x0, long y0, int w, int h, LogOddsCell[] cells)
        {
            if (cells == null || w < 1 || h < 1 || cells.LongLength != (long)w * h)
                throw new ArgumentException("WorldPut: cells must hold w * h cells");
            long dropped;
            fixed (LogOddsCell* p = cells)
                Native.Check(Native.slamhip_hs_world_cells_upload(Pyramid.Ptr, level, x0, y0, w, h, p, out dropped));
            MarkStale();
            return dropped;
        }

        /// <summary>The extents of the world on `level`, in WORLD cells, over the cells whose Value != 0 in the window and in every
        /// tile (slamhip_hs_world_extends); false, and zeros, if there is none.</summary>
        public unsafe bool WorldExtends(int level, out long xMax, out long yMax, out long xMin, out long yMin)
        {
            long* e = stackalloc long[4];
            Native.Check(Native.slamhip_hs_world_extends(Pyramid.Ptr, level, e, out int found));
            xMax = e[0]; yMax = e[1]; xMin = e[2]; yMin = e[3];
            return found != 0;
        }

        private const ulong WorldMagic = 0x31444C524F574853UL;          // "SHWORLD1"
        private const int WorldBandCells = 1 << 26;                      // the bound of one world download / upload

        /// <summary>The world as one raw little-endian file (this shim's own format, not the Python binding's .npz): the magic
        /// "SHWORLD1"; float cell length of level 0; int32 level-0 width, height, levels; int64 origin x, y; int32 tile and uint64
        /// max_bytes of the backing setting (zeros: off); then per level int64 x0, y0 and int32 w, h of the WorldExtends rectangle
        /// (all zero for an empty level) followed by its w * h cells {int32 UpdateIndex, float Value}, row-major.</summary>
        public void SaveWorld(string path)
        {
            using var f = new System.IO.BinaryWriter(System.IO.File.Create(path));
            BackingStats st = BackingStats;
            (long ox, long oy) = Origin;
            f.Write(WorldMagic); f.Write(Maps[0].Properties.CellLength);
            f.Write(Maps[0].Dimensions.X); f.Write(Maps[0].Dimensions.Y); f.Write(NumLevels);
            f.Write(ox); f.Write(oy); f.Write(st.Tile); f.Write((ulong)st.CapacityBytes);
            for (int l = 0; l < NumLevels; l++)
            {
                if (!WorldExtends(l, out long xMax, out long yMax, out long xMin, out long yMin))
                {
                    f.Write(0L); f.Write(0L); f.Write(0); f.Write(0);
                    continue;
                }
                int w = checked((int)(xMax - xMin + 1)), h = checked((int)(yMax - yMin + 1));
                f.Write(xMin); f.Write(yMin); f.Write(w); f.Write(h);
                int rows = Math.Max(1, WorldBandCells / w);
                for (int r = 0; r < h; r += rows)
                    f.Write(MemoryMarshal.AsBytes(WorldCells(l, xMin, yMin + r, w, Math.Min(rows, h - r)).AsSpan()));
            }
        }

        /// <summary>Resume from a file SaveWorld wrote: a geometry that differs from this pyramid's is refused before anything
        /// changes; the window is shifted to the saved origin (through `shift` if given: HectorSLAMProcessor.LoadWorld keeps its poses
        /// world poses that way); backing is switched on with the saved setting if it is off here and was on there; every level's
        /// rectangle is put back with WorldPut.  Returns the cells dropped.</summary>
        public long LoadWorld(string path, Action<int, int> shift = null)
        {
            using var f = new System.IO.BinaryReader(System.IO.File.OpenRead(path));
            if (f.ReadUInt64() != WorldMagic) throw new System.IO.InvalidDataException("LoadWorld: not a SHWORLD1 file");
            float cell = f.ReadSingle();
            int w0 = f.ReadInt32(), h0 = f.ReadInt32(), levels = f.ReadInt32();
            if (BitConverter.SingleToInt32Bits(cell) != BitConverter.SingleToInt32Bits(Maps[0].Properties.CellLength) ||
                w0 != Maps[0].Dimensions.X || h0 != Maps[0].Dimensions.Y || levels != NumLevels)
                throw new System.IO.InvalidDataException($"LoadWorld: the saved pyramid ({cell}, {w0} x {h0} x {levels}) is not this one");
            long sox = f.ReadInt64(), soy = f.ReadInt64();
            int tile = f.ReadInt32();
            ulong maxBytes = f.ReadUInt64();
            int g = 1 << (NumLevels - 1), step = (1 << 30) / g * g;      // (slamhip_hs_shift takes 32-bit moves)
            for ((long ox, long oy) = Origin; ox != sox || oy != soy; (ox, oy) = Origin)
            {
                int dx = (int)Math.Clamp(sox - ox, -step, step), dy = (int)Math.Clamp(soy - oy, -step, step);
                if (shift != null) shift(dx, dy); else Shift(dx, dy);
            }
            if (maxBytes > 0 && BackingStats.On == 0) SetBacking(tile, maxBytes);   // (after the move: an empty window makes no tiles)
            long dropped = 0;
            for (int l = 0; l < NumLevels; l++)
            {
                long x0 = f.ReadInt64(), y0 = f.ReadInt64();
                int w = f.ReadInt32(), h = f.ReadInt32();
                if (w == 0 || h == 0) continue;
                int rows = Math.Max(1, WorldBandCells / w);
                for (int r = 0; r < h; r += rows)
                {
                    int n = Math.Min(rows, h - r);
                    var cells = new LogOddsCell[(long)w * n];
                    Span<byte> rest = MemoryMarshal.AsBytes(cells.AsSpan());
                    while (rest.Length > 0)                             // (Stream.Read may return less than it was asked for)
                    {
                        int got = f.BaseStream.Read(rest);
                        if (got <= 0) throw new System.IO.EndOfStreamException("LoadWorld: the file ends inside level " + l);
                        rest = rest.Slice(got);
                    }
                    dropped += WorldPut(l, x0, y0 + r, w, n, cells);
                }
            }
            MarkStale();
            return dropped;
        }

        /// <summary>The device maps changed behind this object's back (HectorSLAMProcessor.Update drives the native processor): host mirrors are stale.</summary>
        internal void MarkStale()
        {
            foreach (OccGridMap m in Maps) m.mirrorStale = true;
        }

        // The reference reads the scan at call time (ScanMatcher.cs:149-195, OccGridMap.cs:114-239): a caller may refill one
        // ScanCloud in place, or change its Pose, between two calls.  Every call therefore hands the scan to the library again --
        // slamhip_hs_set_scan is a host memcpy into a pinned staging block; the upload itself is deferred to the first kernel that
        // reads the points, so matching and then updating with one scan still uploads it once per call pair at most.
        internal unsafe void SetScan(ScanCloud scan)
        {
            fixed (Vector2* p = CollectionsMarshal.AsSpan(scan.Points))
                Native.Check(Native.slamhip_hs_set_scan(Pyramid.Ptr, p, scan.Points.Count, new Vector2(scan.Pose.X, scan.Pose.Y)));
        }

        public void SetUpdateFactorFree(float factor)                    // MapRepMultiMap.cs:83-89
        {
            foreach (OccGridMap m in Maps) m.SetFactorsSilently(factor, m.UpdateOccupiedFactor);
            Native.Check(Native.slamhip_hs_set_factors(Pyramid.Ptr, factor, Maps[0].UpdateOccupiedFactor));
        }

        public void SetUpdateFactorOccupied(float factor)                // MapRepMultiMap.cs:92-95
        {
            foreach (OccGridMap m in Maps) m.SetFactorsSilently(m.UpdateFreeFactor, factor);
            Native.Check(Native.slamhip_hs_set_factors(Pyramid.Ptr, Maps[0].UpdateFreeFactor, factor));
        }

        public void Dispose()
        {
            Pyramid.Dispose();
            if (ownsDevice) Device.Dispose();
            GC.SuppressFinalize(this);
        }
    }
}
