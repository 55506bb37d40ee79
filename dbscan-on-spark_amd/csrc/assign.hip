// assign.hip -- out-of-sample assignment: a core-point index over a fitted model and the
// kernels that label new points against it (include/dbscan_hip.h, "Out-of-sample assignment").
//
// A query takes the label the Archery border rule (LocalDBSCANArchery.scala:103-106) would give
// a non-core point at its position: the smallest cluster id among the model's cores within eps
// under the reference's exact predicate (DBSCANPoint.scala:26-30), Noise when there is none.
//
// Index (dbscan_index, internal.h): the cores compacted out of the model, binned on a uniform
// grid of side >= eps over their bounding box, radix-sorted by cell key (tile << 6 | local cell,
// tiles of 8x8 cells row-major) and stored as AoS records; a dense tile map (64-bit occupancy
// mask + first occupied-cell ordinal per tile) resolves any cell with one popcount, whatever the
// grid size.  The grid is coarsened until its tile map fits kAssignMaxTiles: a 3x3 stencil is
// correct for any side >= eps, a coarser grid only tests more candidates.
//
// Assign: one query per lane.  Large batches are binned on the same grid and sorted, so the 64
// lanes of a wave walk the same few cells and their record loads hit the same lines; small
// batches skip the sort.  Each of the three stencil rows is at most two contiguous record ranges
// (cells of one tile row are consecutive in key order).  The result of a query is a minimum over
// a set, so it does not depend on the order queries or candidates are visited in: both forms
// agree bit for bit.
#include "internal.h"

#include <cmath>
#include <cstring>
#include <vector>

// the predicate must stay mul, mul, add, compare (the Makefile passes -ffp-contract=off too)
#pragma clang fp contract(off)

namespace dbscan {

namespace {

constexpr int kAssignBlock = 256;

enum AssignMisc { kAmBadCore = 0, kAmMaxCluster = 1, kAmCores = 2, kAmCells = 3, kAmCount = 4 };

// The cell of a coordinate on the index grid, for cores and queries alike: false when the
// coordinate is NaN or lies more than one cell outside [0, ncell) (such a query has no core in
// its stencil); else *c in [-1, ncell].
//
// Why |q - c| <= eps puts the cells of q and c at most 1 apart.  t(v) = fl(fl(v/2 - vmin/2) *
// inv2) with v/2 and vmin/2 exact, so t(v) = (v - vmin) * inv * (1 + d), |d| <= 2^-52, where
// inv = inv2 / 2 = 1 / (side * (1 + 2^-20)) and side >= |eps|.  A pair that passes the predicate
// has fl(dx * dx) <= fl(eps * eps), hence |q - c| <= |eps| * (1 + 2^-50).  Then
//   |t(q) - t(c)| <= |q - c| * inv + 2^-52 * (|t(q)| + |t(c)|)
//                 <= (1 + 2^-50) / (1 + 2^-20) + 2^-52 * 2 * (2^23 + 2)  <  1 - 2^-21 + 2^-27 < 1
// (an axis has at most 8 * kAssignMaxTiles = 2^23 cells; a matching q has |t(q)| <= |t(c)| + 1).
// floor is exact and monotone, so the cell indices differ by at most 1.  The same bound shows a
// query rejected here (t < -1 or t >= ncell + 1, while every core has 0 <= t < ncell) matches no
// core.  The conversion happens after the range check in double, so it never overflows.
__device__ __forceinline__ bool assign_cell(double v, double vmin2, double inv2, int32_t ncell,
                                            int32_t* c) {
    const double t = (v * 0.5 - vmin2) * inv2;
    if (!(t >= -1.0 && t < (double)ncell + 1.0)) return false;
    *c = (int32_t)floor(t);
    return true;
}

__device__ __forceinline__ uint32_t assign_key(int32_t cx, int32_t cy, const AssignGrid& g) {
    cx = cx < 0 ? 0 : (cx >= g.nx ? g.nx - 1 : cx);
    cy = cy < 0 ? 0 : (cy >= g.ny ? g.ny - 1 : cy);
    const uint32_t tile = (uint32_t)(cy >> 3) * (uint32_t)g.ntx + (uint32_t)(cx >> 3);
    return (tile << 6) | (uint32_t)((cy & 7) << 3) | (uint32_t)(cx & 7);
}

// keep[i] = 1 for the cores the index holds; the largest core cluster id and a flag for a core
// without a cluster, reduced per wave before the atomics.
__global__ __launch_bounds__(kAssignBlock) void index_mark_kernel(
    const double* __restrict__ x, const double* __restrict__ y,
    const int32_t* __restrict__ cluster, const uint8_t* __restrict__ flag, int64_t n,
    int all_pairs, int no_pairs, uint8_t* __restrict__ keep, int32_t* __restrict__ misc) {
    const int64_t i = (int64_t)blockIdx.x * kAssignBlock + threadIdx.x;
    int32_t mx = 0, bad = 0;
    if (i < n) {
        const bool core = flag[i] == DBSCAN_FLAG_CORE;
        bool k = false;
        if (core) {
            const int32_t c = cluster[i];
            bad = c <= 0;
            mx = c;
            k = !no_pairs &&
                (all_pairs || (__builtin_isfinite(x[i]) && __builtin_isfinite(y[i])));
        }
        keep[i] = k ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int32_t v = __shfl_xor(mx, o, 64);
        mx = v > mx ? v : mx;
        bad |= __shfl_xor(bad, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (mx > 0) atomicMax(&misc[kAmMaxCluster], mx);
        if (bad) atomicOr(&misc[kAmBadCore], 1);
    }
}

__global__ __launch_bounds__(kAssignBlock) void index_compact_kernel(
    const double* __restrict__ x, const double* __restrict__ y,
    const int32_t* __restrict__ cluster, const uint8_t* __restrict__ keep,
    const int32_t* __restrict__ pos, int64_t n, double* __restrict__ cx, double* __restrict__ cy,
    int32_t* __restrict__ cl, int32_t* __restrict__ id) {
    const int64_t i = (int64_t)blockIdx.x * kAssignBlock + threadIdx.x;
    if (i >= n || !keep[i]) return;
    const int32_t p = pos[i];
    cx[p] = x[i];
    cy[p] = y[i];
    cl[p] = cluster[i];
    id[p] = (int32_t)i;
}

// Sort keys of points on the index grid (cores: every one is inside; queries: clamped, the key
// only orders them), and the key width for the sort.
__global__ __launch_bounds__(kAssignBlock) void assign_key_kernel(
    const double* __restrict__ x, const double* __restrict__ y, int64_t n, AssignGrid g,
    uint32_t* __restrict__ key, int32_t* __restrict__ bits_out, int32_t bits) {
    const int64_t i = (int64_t)blockIdx.x * kAssignBlock + threadIdx.x;
    if (i == 0 && bits_out) *bits_out = bits;
    if (i >= n) return;
    int32_t cx = 0, cy = 0;
    uint32_t k = 0;
    if (assign_cell(x[i], g.xmin2, g.inv2, g.nx, &cx) &&
        assign_cell(y[i], g.ymin2, g.inv2, g.ny, &cy))
        k = assign_key(cx, cy, g);
    key[i] = k;
}

// Records in sorted order (perm == nullptr: in compacted order, the all-pairs index).
__global__ __launch_bounds__(kAssignBlock) void index_pack_kernel(
    const double* __restrict__ cx, const double* __restrict__ cy, const int32_t* __restrict__ cl,
    const int32_t* __restrict__ id, const int32_t* __restrict__ perm, int64_t nc,
    double2* __restrict__ xy, int2* __restrict__ ci) {
    const int64_t k = (int64_t)blockIdx.x * kAssignBlock + threadIdx.x;
    if (k >= nc) return;
    const int64_t j = perm ? perm[k] : k;
    xy[k] = make_double2(cx[j], cy[j]);
    ci[k] = make_int2(cl[j], id[j]);
}

__global__ __launch_bounds__(kAssignBlock) void index_head_kernel(const uint32_t* __restrict__ key,
                                                                  int64_t nc,
                                                                  uint8_t* __restrict__ head) {
    const int64_t k = (int64_t)blockIdx.x * kAssignBlock + threadIdx.x;
    if (k >= nc) return;
    head[k] = (k == 0 || key[k] != key[k - 1]) ? 1 : 0;
}

// The occupied cells' first records and the tile map (zeroed before).
__global__ __launch_bounds__(kAssignBlock) void index_cells_kernel(
    const uint32_t* __restrict__ key, const uint8_t* __restrict__ head,
    const int32_t* __restrict__ ord, int64_t nc, int64_t ntiles, int32_t* __restrict__ cstart,
    AssignTile* __restrict__ tmap) {
    const int64_t k = (int64_t)blockIdx.x * kAssignBlock + threadIdx.x;
    if (k >= nc) return;
    const int32_t o = ord[k];
    if (head[k]) {
        const uint32_t kk = key[k];
        const uint32_t tile = kk >> 6;
        if ((int64_t)tile < ntiles) {  // (always: keys come from assign_key on this grid)
            cstart[o] = (int32_t)k;
            atomicOr((unsigned long long*)&tmap[tile].mask, 1ull << (kk & 63u));
            if (k == 0 || (key[k - 1] >> 6) != tile) tmap[tile].base = o;
        }
    }
    if (k == nc - 1) cstart[o + (head[k] ? 1 : 0)] = (int32_t)nc;
}

struct Best {
    int32_t cl, id;
    double d2;
};

// The reference's predicate on one candidate record, and the running minima.
__device__ __forceinline__ void assign_test(double qx, double qy, double eps2, const double2 p,
                                            const int2* __restrict__ ci, int64_t j, Best& b) {
    const double dx = p.x - qx;
    const double dy = p.y - qy;
    const double d2 = dx * dx + dy * dy;
    if (d2 <= eps2) {
        const int2 c = ci[j];
        if (b.id < 0 || c.x < b.cl) b.cl = c.x;
        if (b.id < 0 || d2 < b.d2 || (d2 == b.d2 && c.y < b.id)) {
            b.d2 = d2;
            b.id = c.y;
        }
    }
}

__device__ __forceinline__ void assign_store(const Best& b, int64_t q,
                                             int32_t* __restrict__ cluster,
                                             uint8_t* __restrict__ flag,
                                             int32_t* __restrict__ nearest) {
    cluster[q] = b.id >= 0 ? b.cl : 0;
    flag[q] = b.id >= 0 ? DBSCAN_FLAG_BORDER : DBSCAN_FLAG_NOISE;
    if (nearest) nearest[q] = b.id;
}

// One query per lane over the 3x3 stencil of its cell.  SORTED: lane t takes the query
// perm[t] (queries sorted by cell key); else query t.  Compiles to 43 VGPRs, no scratch
// (8 waves per SIMD at 256 threads): the plain launch bound is the right one.
template <bool SORTED>
__global__ __launch_bounds__(kAssignBlock) void assign_kernel(
    const double* __restrict__ qx, const double* __restrict__ qy, int64_t m,
    const int32_t* __restrict__ perm, AssignGrid g, double eps2, int64_t ncells,
    const double2* __restrict__ xy, const int2* __restrict__ ci,
    const int32_t* __restrict__ cstart, const AssignTile* __restrict__ tmap,
    int32_t* __restrict__ cluster, uint8_t* __restrict__ flag, int32_t* __restrict__ nearest) {
    const int64_t t = (int64_t)blockIdx.x * kAssignBlock + threadIdx.x;
    if (t >= m) return;
    const int64_t q = SORTED ? (int64_t)perm[t] : t;
    const double x = qx[q], y = qy[q];
    Best b{0, -1, 0.0};
    int32_t cx, cy;
    if (assign_cell(x, g.xmin2, g.inv2, g.nx, &cx) && assign_cell(y, g.ymin2, g.inv2, g.ny, &cy)) {
        const int32_t r0 = cy - 1 < 0 ? 0 : cy - 1, r1 = cy + 1 > g.ny - 1 ? g.ny - 1 : cy + 1;
        const int32_t a0 = cx - 1 < 0 ? 0 : cx - 1, a1 = cx + 1 > g.nx - 1 ? g.nx - 1 : cx + 1;
        for (int32_t r = r0; r <= r1; ++r) {
            // the row's <= 3 cells: one piece per tile they fall in (<= 2)
            for (int32_t c0 = a0; c0 <= a1;) {
                const int32_t tx = c0 >> 3;
                const int32_t ce = a1 < tx * 8 + 7 ? a1 : tx * 8 + 7;
                const AssignTile te = tmap[(int64_t)(r >> 3) * g.ntx + tx];
                const int b0 = ((r & 7) << 3) | (c0 & 7);
                const uint64_t sel = ((1ull << (ce - c0 + 1)) - 1ull) << b0;
                const uint64_t hit = te.mask & sel;
                if (hit) {
                    int64_t first = te.base + __popcll(te.mask & ((1ull << b0) - 1ull));
                    int64_t last = first + __popcll(hit);
                    // (a consistent index keeps both within [0, ncells]; never read past it)
                    first = first < 0 ? 0 : (first > ncells ? ncells : first);
                    last = last < first ? first : (last > ncells ? ncells : last);
                    const int32_t s = cstart[first], e = cstart[last];
                    int32_t j = s;
                    for (; j + 4 <= e; j += 4) {  // four record loads in flight per trip
                        const double2 p0 = xy[j], p1 = xy[j + 1], p2 = xy[j + 2], p3 = xy[j + 3];
                        assign_test(x, y, eps2, p0, ci, j, b);
                        assign_test(x, y, eps2, p1, ci, j + 1, b);
                        assign_test(x, y, eps2, p2, ci, j + 2, b);
                        assign_test(x, y, eps2, p3, ci, j + 3, b);
                    }
                    for (; j < e; ++j) assign_test(x, y, eps2, xy[j], ci, j, b);
                }
                c0 = ce + 1;
            }
        }
    }
    assign_store(b, q, cluster, flag, nearest);
}

// eps*eps = +inf: every core against every query (all lanes read the same record).
__global__ __launch_bounds__(kAssignBlock) void assign_all_pairs_kernel(
    const double* __restrict__ qx, const double* __restrict__ qy, int64_t m, double eps2,
    int64_t nc, const double2* __restrict__ xy, const int2* __restrict__ ci,
    int32_t* __restrict__ cluster, uint8_t* __restrict__ flag, int32_t* __restrict__ nearest) {
    const int64_t q = (int64_t)blockIdx.x * kAssignBlock + threadIdx.x;
    if (q >= m) return;
    const double x = qx[q], y = qy[q];
    Best b{0, -1, 0.0};
    for (int64_t j = 0; j < nc; ++j) assign_test(x, y, eps2, xy[j], ci, j, b);
    assign_store(b, q, cluster, flag, nearest);
}

// No cores, or eps*eps NaN: every query is Noise.
__global__ __launch_bounds__(kAssignBlock) void assign_fill_kernel(int64_t m,
                                                                   int32_t* __restrict__ cluster,
                                                                   uint8_t* __restrict__ flag,
                                                                   int32_t* __restrict__ nearest) {
    const int64_t q = (int64_t)blockIdx.x * kAssignBlock + threadIdx.x;
    if (q >= m) return;
    cluster[q] = 0;
    flag[q] = DBSCAN_FLAG_NOISE;
    if (nearest) nearest[q] = -1;
}

inline dim3 blocks_for(int64_t n) { return dim3((unsigned)((n + kAssignBlock - 1) / kAssignBlock)); }

// Cells per axis of a core extent on a grid of this side -- the expression assign_cell
// evaluates for the largest coordinate.
inline double axis_cells(double vmax, double vmin2, double inv2) {
    return floor((vmax * 0.5 - vmin2) * inv2) + 1.0;
}

// The grid over the cores' bounding box: side = |eps| * (1 + 2^-20) (the margin assign_cell's
// argument needs), grown until the tile map fits the budget.
AssignGrid size_grid(double xmin, double xmax, double ymin, double ymax, double eps) {
    AssignGrid g{};
    g.xmin2 = xmin * 0.5;
    g.ymin2 = ymin * 0.5;
    const double hx = xmax * 0.5 - g.xmin2, hy = ymax * 0.5 - g.ymin2;  // half extents: finite
    double side = fabs(eps) * (1.0 + 0x1p-20);
    if (!(side >= 1e-300)) side = 1e-300;  // eps ~ 0: any side >= eps will do; keep 1/side finite
    // no axis longer than the whole budget (half extents, so nothing overflows)
    const double axis_side = (hx > hy ? hx : hy) / (4.0 * (double)kAssignMaxTiles - 1.0);
    if (axis_side > side) side = axis_side;
    for (int it = 0; it < 400; ++it) {
        const double inv2 = 2.0 / side;
        const double nx = axis_cells(xmax, g.xmin2, inv2), ny = axis_cells(ymax, g.ymin2, inv2);
        const double tiles = ceil(nx / 8.0) * ceil(ny / 8.0);
        if (std::isfinite(inv2) && tiles <= (double)kAssignMaxTiles) {
            g.inv2 = inv2;
            g.nx = (int32_t)nx;
            g.ny = (int32_t)ny;
            g.ntx = (g.nx + 7) / 8;
            g.nty = (g.ny + 7) / 8;
            return g;
        }
        // coarsen by the excess in area (a thin grid shrinks along one axis only: iterate)
        double f = sqrt(tiles / (double)kAssignMaxTiles);
        if (!(f >= 1.0) || !std::isfinite(f)) f = 2.0;
        side *= f * 1.01;
        if (!std::isfinite(side)) break;
    }
    throw ArgError{"the index grid could not be sized"};
}

}  // namespace

void build_index(hipStream_t s, Workspace& ws, Profiler* prof, const double* x, const double* y,
                 const int32_t* cluster, const uint8_t* flag, int64_t n, double eps,
                 dbscan_index* idx) {
    const double eps2 = eps * eps;
    idx->n = n;
    idx->eps2 = eps2;
    idx->mode = 2;
    if (n == 0) return;
    const int no_pairs = std::isnan(eps2), all_pairs = std::isinf(eps2);

    int32_t* misc = static_cast<int32_t*>(ws.a_misc.ensure(kAmCount * sizeof(int32_t)));
    // (sized for the bbox partials too: the buffer must not move while kernels read it)
    const size_t tmp_bytes = (size_t)n > 1024 * 5 * sizeof(double) ? (size_t)n
                                                                   : 1024 * 5 * sizeof(double);
    uint8_t* keep = static_cast<uint8_t*>(ws.a_tmp.ensure(tmp_bytes));
    int32_t* pos = static_cast<int32_t*>(ws.a_val.ensure((size_t)n * sizeof(int32_t)));
    DBSCAN_HIP_CHECK(hipMemsetAsync(misc, 0, kAmCount * sizeof(int32_t), s));
    klaunch(prof, "index_mark", index_mark_kernel, blocks_for(n), dim3(kAssignBlock), 0, s, x, y,
            cluster, flag, n, all_pairs, no_pairs, keep, misc);
    DBSCAN_HIP_CHECK(hipGetLastError());
    exclusive_scan(s, 1, keep, pos, n, misc + kAmCores, ws.ascan);
    int32_t hm[kAmCount];
    DBSCAN_HIP_CHECK(hipMemcpyAsync(hm, misc, sizeof(hm), hipMemcpyDeviceToHost, s));
    DBSCAN_HIP_CHECK(hipStreamSynchronize(s));
    if (hm[kAmBadCore]) throw ArgError{"a Core point of the model has cluster <= 0"};
    idx->max_cluster = hm[kAmMaxCluster];
    const int64_t nc = hm[kAmCores];
    if (nc == 0) return;

    double* cx = static_cast<double*>(ws.a_cx.ensure((size_t)nc * sizeof(double)));
    double* cy = static_cast<double*>(ws.a_cy.ensure((size_t)nc * sizeof(double)));
    int32_t* cl = static_cast<int32_t*>(ws.a_cl.ensure((size_t)nc * sizeof(int32_t)));
    int32_t* id = static_cast<int32_t*>(ws.a_id.ensure((size_t)nc * sizeof(int32_t)));
    klaunch(prof, "index_compact", index_compact_kernel, blocks_for(n), dim3(kAssignBlock), 0, s,
            x, y, cluster, (const uint8_t*)keep, (const int32_t*)pos, n, cx, cy, cl, id);
    DBSCAN_HIP_CHECK(hipGetLastError());
    double2* xy = static_cast<double2*>(idx->xy.ensure((size_t)nc * sizeof(double2)));
    int2* ci = static_cast<int2*>(idx->ci.ensure((size_t)nc * sizeof(int2)));
    if (all_pairs) {
        klaunch(prof, "index_pack", index_pack_kernel, blocks_for(nc), dim3(kAssignBlock), 0, s,
                (const double*)cx, (const double*)cy, (const int32_t*)cl, (const int32_t*)id,
                (const int32_t*)nullptr, nc, xy, ci);
        DBSCAN_HIP_CHECK(hipGetLastError());
        DBSCAN_HIP_CHECK(hipStreamSynchronize(s));
        idx->ncores = nc;
        idx->mode = 1;
        return;
    }

    // the cores' bounding box (every one finite here) and the grid over it
    double* partial = nullptr;
    const int nb = bbox_partials(s, cx, cy, nc, ws.a_tmp, &partial);  // (keep is consumed)
    std::vector<double> hp((size_t)nb * 5);
    DBSCAN_HIP_CHECK(hipMemcpyAsync(hp.data(), partial, hp.size() * sizeof(double),
                                    hipMemcpyDeviceToHost, s));
    DBSCAN_HIP_CHECK(hipStreamSynchronize(s));
    double xmin = INFINITY, xmax = -INFINITY, ymin = INFINITY, ymax = -INFINITY;
    for (int b = 0; b < nb; ++b) {
        xmin = fmin(xmin, hp[(size_t)b * 5]);
        xmax = fmax(xmax, hp[(size_t)b * 5 + 1]);
        ymin = fmin(ymin, hp[(size_t)b * 5 + 2]);
        ymax = fmax(ymax, hp[(size_t)b * 5 + 3]);
    }
    if (!(xmin <= xmax && ymin <= ymax)) throw ArgError{"the index found no finite core"};
    const AssignGrid g = size_grid(xmin, xmax, ymin, ymax, eps);
    const int64_t ntiles = (int64_t)g.ntx * g.nty;
    int32_t bits = 6;
    while ((int64_t(1) << bits) < ntiles * 64) ++bits;

    uint32_t* key = static_cast<uint32_t*>(ws.a_key.ensure((size_t)nc * sizeof(uint32_t)));
    uint32_t* key2 = static_cast<uint32_t*>(ws.a_key2.ensure((size_t)nc * sizeof(uint32_t)));
    uint32_t* key3 = static_cast<uint32_t*>(ws.a_key3.ensure((size_t)nc * sizeof(uint32_t)));
    int32_t* val = static_cast<int32_t*>(ws.a_val.ensure((size_t)nc * sizeof(int32_t)));
    int32_t* val2 = static_cast<int32_t*>(ws.a_val2.ensure((size_t)nc * sizeof(int32_t)));
    int32_t* val3 = static_cast<int32_t*>(ws.a_val3.ensure((size_t)nc * sizeof(int32_t)));
    int32_t* bits_dev = static_cast<int32_t*>(idx->bits.ensure(sizeof(int32_t)));
    klaunch(prof, "assign_key", assign_key_kernel, blocks_for(nc), dim3(kAssignBlock), 0, s,
            (const double*)cx, (const double*)cy, nc, g, key, bits_dev, bits);
    DBSCAN_HIP_CHECK(hipGetLastError());
    radix_sort_pairs(s, key, val, key2, val2, key3, val3, nc, bits_dev, ws.a_hist, ws.ascan, prof,
                     nullptr, true);
    klaunch(prof, "index_pack", index_pack_kernel, blocks_for(nc), dim3(kAssignBlock), 0, s,
            (const double*)cx, (const double*)cy, (const int32_t*)cl, (const int32_t*)id,
            (const int32_t*)val, nc, xy, ci);
    DBSCAN_HIP_CHECK(hipGetLastError());

    // occupied cells and the tile map (head flags in a_tmp, their ordinals in val2)
    uint8_t* head = static_cast<uint8_t*>(ws.a_tmp.ensure((size_t)nc));
    int32_t* ord = val2;
    int32_t* cstart = static_cast<int32_t*>(idx->cstart.ensure((size_t)(nc + 1) * sizeof(int32_t)));
    AssignTile* tmap =
        static_cast<AssignTile*>(idx->tmap.ensure((size_t)ntiles * sizeof(AssignTile)));
    DBSCAN_HIP_CHECK(hipMemsetAsync(tmap, 0, (size_t)ntiles * sizeof(AssignTile), s));
    klaunch(prof, "index_head", index_head_kernel, blocks_for(nc), dim3(kAssignBlock), 0, s,
            (const uint32_t*)key, nc, head);
    DBSCAN_HIP_CHECK(hipGetLastError());
    exclusive_scan(s, 1, head, ord, nc, misc + kAmCells, ws.ascan);
    klaunch(prof, "index_cells", index_cells_kernel, blocks_for(nc), dim3(kAssignBlock), 0, s,
            (const uint32_t*)key, (const uint8_t*)head, (const int32_t*)ord, nc, ntiles, cstart,
            tmap);
    DBSCAN_HIP_CHECK(hipGetLastError());
    int32_t ncells = 0;
    DBSCAN_HIP_CHECK(hipMemcpyAsync(&ncells, misc + kAmCells, sizeof(int32_t),
                                    hipMemcpyDeviceToHost, s));
    DBSCAN_HIP_CHECK(hipStreamSynchronize(s));
    idx->g = g;
    idx->ncores = nc;
    idx->ncells = ncells;
    idx->mode = 0;
}

void enqueue_assign(hipStream_t s, Workspace& ws, Profiler* prof, const dbscan_index* idx,
                    const double* qx, const double* qy, int64_t m, int32_t* cluster,
                    uint8_t* flag, int32_t* nearest, int64_t sort_min) {
    if (m <= 0) return;
    if (idx->mode == 2) {
        klaunch(prof, "assign_fill", assign_fill_kernel, blocks_for(m), dim3(kAssignBlock), 0, s, m,
                cluster, flag, nearest);
        DBSCAN_HIP_CHECK(hipGetLastError());
        return;
    }
    const double2* xy = static_cast<const double2*>(idx->xy.p);
    const int2* ci = static_cast<const int2*>(idx->ci.p);
    if (idx->mode == 1) {
        klaunch(prof, "assign_all_pairs", assign_all_pairs_kernel, blocks_for(m),
                dim3(kAssignBlock), 0, s, qx, qy, m, idx->eps2, idx->ncores, xy, ci, cluster, flag,
                nearest);
        DBSCAN_HIP_CHECK(hipGetLastError());
        return;
    }
    const int32_t* cstart = static_cast<const int32_t*>(idx->cstart.p);
    const AssignTile* tmap = static_cast<const AssignTile*>(idx->tmap.p);
    if (m < sort_min) {
        klaunch(prof, "assign_direct", assign_kernel<false>, blocks_for(m), dim3(kAssignBlock), 0,
                s, qx, qy, m, (const int32_t*)nullptr, idx->g, idx->eps2, idx->ncells, xy, ci,
                cstart, tmap, cluster, flag, nearest);
        DBSCAN_HIP_CHECK(hipGetLastError());
        return;
    }
    uint32_t* key = static_cast<uint32_t*>(ws.a_key.ensure((size_t)m * sizeof(uint32_t)));
    uint32_t* key2 = static_cast<uint32_t*>(ws.a_key2.ensure((size_t)m * sizeof(uint32_t)));
    uint32_t* key3 = static_cast<uint32_t*>(ws.a_key3.ensure((size_t)m * sizeof(uint32_t)));
    int32_t* val = static_cast<int32_t*>(ws.a_val.ensure((size_t)m * sizeof(int32_t)));
    int32_t* val2 = static_cast<int32_t*>(ws.a_val2.ensure((size_t)m * sizeof(int32_t)));
    int32_t* val3 = static_cast<int32_t*>(ws.a_val3.ensure((size_t)m * sizeof(int32_t)));
    klaunch(prof, "assign_key", assign_key_kernel, blocks_for(m), dim3(kAssignBlock), 0, s, qx, qy,
            m, idx->g, key, (int32_t*)nullptr, 0);
    DBSCAN_HIP_CHECK(hipGetLastError());
    radix_sort_pairs(s, key, val, key2, val2, key3, val3, m,
                     static_cast<const int32_t*>(idx->bits.p), ws.a_hist, ws.ascan, prof, nullptr,
                     true);
    klaunch(prof, "assign_sorted", assign_kernel<true>, blocks_for(m), dim3(kAssignBlock), 0, s, qx,
            qy, m, (const int32_t*)val, idx->g, idx->eps2, idx->ncells, xy, ci, cstart, tmap,
            cluster, flag, nearest);
    DBSCAN_HIP_CHECK(hipGetLastError());
}

}  // namespace dbscan
