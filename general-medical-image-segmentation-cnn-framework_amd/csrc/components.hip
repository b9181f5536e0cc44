// components.hip -- connected components of a predicted mask on the device: the clean-up between the aggregated mask (predict.py:139-147)
// and the metrics (predict.py:151/154).  Semantics of scipy.ndimage.label with generate_binary_structure(3, 1 / 2 / 3): foreground is
// != 0, neighbours are the 6 faces, 18 faces + edges or 26 faces + edges + corners, outside the array is background.
//
// Block-based union-find over parent[], an int32 per voxel: -1 on background, on foreground the linear index of another voxel of the
// same component.
//   INVARIANT: parent[i] <= i at all times.  The local kernel stores the minimum index of the voxel's in-tile component; the merge
//   kernel changes parent[] only with atomicMin(&parent[hi], lo) with lo < hi, which can only lower a value.
//   A find therefore walks strictly decreasing indices and ends after at most i steps at a voxel with parent[r] == r; a union that
//   loses its race continues from the value the atomic returned, which is strictly below the index it tried to link, and ends too.
//   A root is <= every voxel below it, so the root of a finished component IS its first voxel in z,y,x raster order: the label
//   root + 1 does not depend on scheduling, and two runs are bitwise equal.
// No workgroup waits for another one anywhere in this file; the only ordering between workgroups is the kernel boundary.
//   components_local    one workgroup per 8 x 8 x 64 tile: union-find of the tile in LDS, parent[] and the per-tile counts out
//   components_merge    the voxels on tile faces join their roots across tiles (device-scope atomics only)
//   components_flatten  labels[v] = root + 1; the per-tile counts move to sizes[root], one atomic per (tile, tile-local component)
//   components_info     foreground voxels, components, largest component (reduction over sizes[])
//   components_filter   out[v] = keep(labels[v]) ? mask[v] : 0, and the number of voxels set to 0
//
// The class-aware form (Cls = true in the local and merge kernels): two voxels join only when they are neighbours AND
// carry the same class 1..255; 0 and every value outside 0..255 is background (the latter counted).  All classes are labelled in one
// call: components of different classes have different first voxels, so parent[], labels[] and sizes[] hold them side by side and
// flatten / info run unchanged.  The local kernel leaves a 1-byte class volume in the workspace for the merge kernel, which reads it
// with plain loads (a kernel boundary lies between the two): one byte per neighbour, not the 8 bytes of a mask value.
//   components_rank_count / _scan / components_table / components_relabel   the compact table of the n components in raster order
//                       of their first voxels (first, size, class) and labels 1..n: an exclusive prefix count of sizes[r] > 0
//   components_filter_table   out[v] = (lc[v] == 0 || keep[lc[v] - 1]) ? mask[v] : 0 with one keep flag per component
#include "common.h"
#include "internal.h"

namespace seg {

constexpr int kCcTZ = 8, kCcTY = 8, kCcTX = 64;         // the tile, z x y x x: 4096 voxels, 32 KiB of LDS
constexpr int kCcThreads = 256;
static_assert(kCcThreads == kReduceThreads, "the block size of reduce.h");
constexpr int kCcWaves = kCcThreads / kWave;
constexpr int kCcRows = kCcTZ * kCcTY;                  // rows of kCcTX = 64 voxels: one wave owns a row at a time
constexpr int kCcRowsPerWave = kCcRows / kCcWaves;
constexpr int kCcTile = kCcRows * kCcTX;
constexpr long long kCcMaxVoxels = (1ll << 31) - 2;     // root + 1 must fit an int32
static_assert(kCcTX == kWave, "a wave owns one row of the tile");
static_assert(kCcRows % kCcWaves == 0, "rows divide among the waves");

static int cc_grid(long long items) { return stream_grid(items, kCcThreads, 4096); }

// ---- union-find on an int array in LDS (workgroup scope) or in global memory (agent scope).
// Every access is an atomic of that scope.  In global memory this is what makes the merge kernel correct across XCDs: the per-XCD
// L2s are not coherent inside a kernel, a device-scope atomicMin is performed where every XCD sees it, and a relaxed agent-scope load
// does not stay in this CU's L1.  A load that still returns an OLDER value of parent[i] is harmless: every value parent[i] ever held
// is a voxel of i's component that is <= i, so a find that ends early hands the union a member of the right set, and the atomicMin
// that follows returns the true value and corrects the walk.
template <int Scope>
__device__ __forceinline__ int uf_find(const int* p, int i) {
    // strictly decreasing (parent[i] <= i), so at most i steps
    for (;;) {
        const int q = __hip_atomic_load(p + i, __ATOMIC_RELAXED, Scope);
        if (q == i) return i;
        i = q;
    }
}

template <int Scope>
__device__ __forceinline__ void uf_union(int* p, int a, int b) {
    // max(a, b) strictly decreases from one turn to the next: `old` < hi and lo < hi
    for (;;) {
        a = uf_find<Scope>(p, a);
        b = uf_find<Scope>(p, b);
        if (a == b) return;
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        const int old = __hip_atomic_fetch_min(p + hi, lo, __ATOMIC_RELAXED, Scope);
        if (old == hi) return;          // hi was a root and now hangs below lo
        // hi was linked meanwhile (or the find read an old value): it now points at min(old, lo); what is left is old ~ lo
        a = old;
        b = lo;
    }
}

// (dz, dy) of the four rows that hold backward neighbours: the row above in the slice, and three rows of the slice before
__constant__ const int kCcRowDz[4] = {0, -1, -1, -1};
__constant__ const int kCcRowDy[4] = {-1, -1, 0, 1};

// how far a row reaches in x under connectivity c: -1 = not a neighbour row, 0 = dx = 0 only, 1 = dx in {-1, 0, 1}
__device__ __forceinline__ int cc_row_reach(int k, int conn) {
    const bool diag = k == 1 || k == 3;          // (dz, dy) both non-zero
    if (conn == 6) return diag ? -1 : 0;
    if (conn == 18) return diag ? 0 : 1;
    return 1;
}

// class of a mask value in the class-aware form: 1..255 as it is; 0, and every value outside 0..255 (counted in `bad`), background
__device__ __forceinline__ int cc_class(int64_t v, int& bad) {
    const bool in = (unsigned long long)v <= 255ull;
    bad += !in;
    return in ? (int)v : 0;
}

// class-aware rows: `bnd` has a bit for every voxel that starts a run of equal non-zero class (non-zero, and lane 0 or another class
// to its left).  The run start of a foreground lane is the highest such bit at or below it (one exists: walk left through equal classes)
__device__ __forceinline__ int cc_run_start(unsigned long long bnd, int lane) {
    return 63 - __clzll((long long)(bnd & (~0ull >> (63 - lane))));
}

// One workgroup per tile.  lab[t] (t = tile-local raster index, the same order as the global raster index) = -1 on background and
// outside the volume, else a tile-local index <= t of the same in-tile component.
// Cls: cnt[] holds the voxel's class (0 = background) through phases 0 and 1, where the binary form leaves it at 0, and is cleared
// behind a barrier before phase 2 counts in it: no third array, the same 32 KiB of LDS.  cvol[] (1 byte per voxel) takes the classes
// for the merge kernel, *oob the voxels of this tile whose value lies outside 0..255 (one integer atomic per workgroup that has any).
template <bool Vec2, bool Cls>
__global__ __launch_bounds__(kCcThreads) void components_local_kernel(const int64_t* __restrict__ mask, int D, int H, int W, int conn,
        int* __restrict__ parent, int* __restrict__ sizes, unsigned char* __restrict__ cvol, unsigned long long* __restrict__ oob) {
    __shared__ int lab[kCcTile];
    __shared__ int cnt[kCcTile];
    const int z0 = blockIdx.z * kCcTZ, y0 = blockIdx.y * kCcTY, x0 = blockIdx.x * kCcTX;
    const long long HW = (long long)H * W;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    int bad = 0;

    // phase 0a: foreground flags.  Vec2: W is even and the mask 16-byte aligned, so voxel pairs (x even) are one 16-byte load
    if (Vec2) {
        for (int p = threadIdx.x; p < kCcTile / 2; p += kCcThreads) {
            const int r = p / (kCcTX / 2), tx = (p - r * (kCcTX / 2)) * 2;
            const int z = z0 + r / kCcTY, y = y0 + r % kCcTY, x = x0 + tx;
            int f0 = -1, f1 = -1, c0 = 0, c1 = 0;
            if (z < D && y < H && x < W) {      // x even and W even: x + 1 < W too
                const longlong2 v = *reinterpret_cast<const longlong2*>(mask + (z * HW + (long long)y * W + x));
                if (Cls) {
                    c0 = cc_class(v.x, bad);
                    c1 = cc_class(v.y, bad);
                    f0 = c0 ? 0 : -1;
                    f1 = c1 ? 0 : -1;
                } else {
                    f0 = v.x != 0 ? 0 : -1;
                    f1 = v.y != 0 ? 0 : -1;
                }
            }
            lab[r * kCcTX + tx] = f0;
            lab[r * kCcTX + tx + 1] = f1;
            cnt[r * kCcTX + tx] = c0;
            cnt[r * kCcTX + tx + 1] = c1;
        }
    } else {
        for (int t = threadIdx.x; t < kCcTile; t += kCcThreads) {
            const int r = t / kCcTX, tx = t - r * kCcTX;
            const int z = z0 + r / kCcTY, y = y0 + r % kCcTY, x = x0 + tx;
            const bool in = z < D && y < H && x < W;
            if (Cls) {
                const int c = in ? cc_class(mask[z * HW + (long long)y * W + x], bad) : 0;
                lab[t] = c ? 0 : -1;
                cnt[t] = c;
            } else {
                lab[t] = (in && mask[z * HW + (long long)y * W + x] != 0) ? 0 : -1;
                cnt[t] = 0;
            }
        }
    }
    __syncthreads();
    // phase 0b: runs along x.  A wave owns a row; every foreground voxel starts at the first voxel of its run, so the x direction
    // needs no union.  Cls: a run is a maximal stretch of EQUAL non-zero class, and the ballot of the run starts is kept beside the
    // foreground bits; the class of the wave's voxel in each row stays in a register for phase 3
    unsigned long long rowbits[kCcRowsPerWave];
    unsigned long long bndbits[Cls ? kCcRowsPerWave : 1];
    int rowcls[Cls ? kCcRowsPerWave : 1];
#pragma unroll
    for (int j = 0; j < kCcRowsPerWave; ++j) {
        const int r = wave + j * kCcWaves;
        if (Cls) {
            const int c = cnt[r * kCcTX + lane];
            const int left = __shfl_up(c, 1, kWave);
            const unsigned long long bits = __ballot(c != 0);
            const unsigned long long bnd = __ballot(c != 0 && (lane == 0 || c != left));
            rowbits[j] = bits;
            bndbits[j] = bnd;
            rowcls[j] = c;
            if (c != 0) lab[r * kCcTX + lane] = r * kCcTX + cc_run_start(bnd, lane);
        } else {
            const bool fg = lab[r * kCcTX + lane] >= 0;
            const unsigned long long bits = __ballot(fg);
            rowbits[j] = bits;
            const unsigned long long zeros_below = ~bits & ((1ull << lane) - 1ull);      // background voxels left of this lane
            const int start = zeros_below ? 64 - __clzll((long long)zeros_below) : 0;
            if (fg) lab[r * kCcTX + lane] = r * kCcTX + start;
        }
    }
    __syncthreads();
    // phase 1: unions with the neighbour rows inside the tile (LDS atomics).  `joins(i)`: voxel i can be joined with t -- foreground,
    // and under Cls of t's class.  Per neighbour row: if the voxel straight across (dx = 0) joins it stands for its whole run, diagonal
    // voxels included (a diagonal voxel that joins is its x neighbour of the same class); the union is skipped when the left voxel of
    // this row and the left voxel across both join, because that pair has joined the same two runs (induction along the run: all four
    // are then of one class).  If the voxel straight across does not join -- background, or under Cls another class -- the diagonal
    // voxels are examined one by one.
    for (int t = threadIdx.x; t < kCcTile; t += kCcThreads) {
        if (lab[t] < 0) continue;
        const int c = Cls ? cnt[t] : 0;
        auto joins = [&](int i) { return Cls ? cnt[i] == c : lab[i] >= 0; };
        const int r = t / kCcTX, tx = t - r * kCcTX, tz = r / kCcTY, ty = r - tz * kCcTY;
        for (int k = 0; k < 4; ++k) {
            const int reach = cc_row_reach(k, conn);
            const int nz = tz + kCcRowDz[k], ny = ty + kCcRowDy[k];
            if (reach < 0 || nz < 0 || ny < 0 || ny >= kCcTY) continue;
            const int nb = (nz * kCcTY + ny) * kCcTX;
            const bool left_in = tx > 0, right_in = tx < kCcTX - 1;
            if (joins(nb + tx)) {
                if (left_in && joins(t - 1) && joins(nb + tx - 1)) continue;
                uf_union<__HIP_MEMORY_SCOPE_WORKGROUP>(lab, t, nb + tx);
            } else if (reach > 0) {
                if (left_in && joins(nb + tx - 1)) uf_union<__HIP_MEMORY_SCOPE_WORKGROUP>(lab, t, nb + tx - 1);
                if (right_in && joins(nb + tx + 1)) uf_union<__HIP_MEMORY_SCOPE_WORKGROUP>(lab, t, nb + tx + 1);
            }
        }
    }
    __syncthreads();
    if (Cls) {                                  // the classes have done their work: cnt[] becomes the counts
        for (int t = threadIdx.x; t < kCcTile; t += kCcThreads) cnt[t] = 0;
        __syncthreads();
    }
    // phase 2: lab[] is read-only now.  The first voxel of each run finds the root and adds the run's length to the root's count:
    // one LDS atomic per run, not per voxel
    int root[kCcRowsPerWave];
#pragma unroll
    for (int j = 0; j < kCcRowsPerWave; ++j) {
        const int r = wave + j * kCcWaves;
        const unsigned long long bits = rowbits[j];
        const bool fg = (bits >> lane) & 1ull;
        int start, rt = -1;
        if (Cls) {
            const unsigned long long bnd = bndbits[j];
            start = fg ? cc_run_start(bnd, lane) : 0;
            if (fg && start == lane) {
                rt = uf_find<__HIP_MEMORY_SCOPE_WORKGROUP>(lab, r * kCcTX + lane);
                const unsigned long long stop = ((~bits | bnd) >> lane) >> 1;   // right of this lane: the next zero or the next run start
                const int len = stop ? __ffsll((long long)stop) : 64 - lane;
                atomicAdd(&cnt[rt], len);
            }
        } else {
            const unsigned long long zeros_below = ~bits & ((1ull << lane) - 1ull);
            start = zeros_below ? 64 - __clzll((long long)zeros_below) : 0;
            if (fg && start == lane) {
                rt = uf_find<__HIP_MEMORY_SCOPE_WORKGROUP>(lab, r * kCcTX + lane);
                const unsigned long long inv = ~(bits >> lane);             // bit 0 is clear; the first set bit ends the run
                const int len = inv ? __ffsll((long long)inv) - 1 : 64;
                atomicAdd(&cnt[rt], len);
            }
        }
        rt = __shfl(rt, start, kWave);
        root[j] = fg ? rt : -1;
    }
    __syncthreads();
    // phase 3: parent[] = global index of the tile-local root, sizes[] = the count at tile-local roots and 0 elsewhere (every voxel of
    // the tile inside the volume is written, so neither array needs clearing); Cls: the class volume likewise
#pragma unroll
    for (int j = 0; j < kCcRowsPerWave; ++j) {
        const int r = wave + j * kCcWaves;
        const int z = z0 + r / kCcTY, y = y0 + r % kCcTY, x = x0 + lane;
        if (z >= D || y >= H || x >= W) continue;
        const long long g = z * HW + (long long)y * W + x;
        const int rt = root[j];
        int pg = -1, c = 0;
        if (rt >= 0) {
            const int rr = rt / kCcTX, rx = rt - rr * kCcTX;
            pg = (int)((z0 + rr / kCcTY) * HW + (long long)(y0 + rr % kCcTY) * W + (x0 + rx));
            if (rt == r * kCcTX + lane) c = cnt[rt];
        }
        parent[g] = pg;
        sizes[g] = c;
        if (Cls) cvol[g] = (unsigned char)rowcls[j];
    }
    if (Cls) {
        // values outside 0..255: the waves' sums (reduce.h's butterfly) meet in four slots of cnt[], which phase 3 has finished with --
        // the helper's own LDS on top of the 32 KiB of the two arrays would cost the fifth workgroup of a CU
        bad = wave_reduce<OpSum>(bad);
        __syncthreads();
        if (lane == 0) cnt[wave] = bad;
        __syncthreads();
        if (threadIdx.x == 0) {
            int all = 0;
            for (int w = 0; w < kCcWaves; ++w) all += cnt[w];
            if (all) atomicAdd(oob, (unsigned long long)all);       // integer, so order-independent
        }
    }
}

// One workgroup per tile.  A foreground voxel on a face of its tile joins its root with the root of every backward neighbour (13 of
// 26, 9 of 18, 3 of 6 offsets: the ones before it in raster order) that lies in ANOTHER tile; pairs inside a tile were joined by the
// local kernel.  Faces, edges and corners of tiles need no cases of their own.  parent[] is touched by device-scope atomics only.
// `joins(i)`: voxel i can be joined with v.  Binary: parent[i] >= 0.  Cls: cvol[i], the class volume of the local kernel, equals v's
// class c != 0 -- "parent[i] >= 0" would join two classes.  cvol[] is read-only in this kernel and was written before it began.
template <bool Cls>
__global__ __launch_bounds__(kCcThreads) void components_merge_kernel(int* parent, const unsigned char* __restrict__ cvol, int D, int H, int W, int conn) {
    const int z0 = blockIdx.z * kCcTZ, y0 = blockIdx.y * kCcTY, x0 = blockIdx.x * kCcTX;
    const long long HW = (long long)H * W;
    for (int t = threadIdx.x; t < kCcTile; t += kCcThreads) {
        const int r = t / kCcTX, tx = t - r * kCcTX, tz = r / kCcTY, ty = r - tz * kCcTY;
        // only these voxels have a backward neighbour outside the tile (dz is never +1)
        if (!(tz == 0 || ty == 0 || ty == kCcTY - 1 || tx == 0 || tx == kCcTX - 1)) continue;
        const int z = z0 + tz, y = y0 + ty, x = x0 + tx;
        if (z >= D || y >= H || x >= W) continue;
        const int v = (int)(z * HW + (long long)y * W + x);
        const int c = Cls ? cvol[v] : 0;
        auto joins = [&](int i) { return Cls ? cvol[i] == c : __hip_atomic_load(parent + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= 0; };
        if (Cls ? c == 0 : !joins(v)) continue;
        const bool left_fg = tx > 0 && joins(v - 1);
        for (int k = 0; k < 13; ++k) {
            // k = 0: (0, 0, -1); k = 1..3: (0, -1, dx); k = 4..12: (-1, dy, dx), dy and dx from -1 to 1
            const int dz = k < 4 ? 0 : -1;
            const int dy = k == 0 ? 0 : (k < 4 ? -1 : (k - 4) / 3 - 1);
            const int dx = k == 0 ? -1 : (k < 4 ? k - 2 : (k - 4) % 3 - 1);
            const int nonzero = (dz != 0) + (dy != 0) + (dx != 0);
            if (nonzero > (conn == 6 ? 1 : conn == 18 ? 2 : 3)) continue;
            const int nz = z + dz, ny = y + dy, nx = x + dx;
            if (nz < 0 || ny < 0 || ny >= H || nx < 0 || nx >= W) continue;                 // outside the array: background
            const bool same_tile = tz + dz >= 0 && ty + dy >= 0 && ty + dy < kCcTY && tx + dx >= 0 && tx + dx < kCcTX;
            if (same_tile) continue;
            const int n = (int)(nz * HW + (long long)ny * W + nx);
            if (!joins(n)) continue;
            // Across a z or y border of the tile the pair one step to the left, (v - 1, n - 1), is a pair of this kernel too (v - 1 lies
            // in this tile on the same face, the offset is the same).  Where both join v (foreground; Cls: all four of one class, v - 1
            // of v's and n - 1 of n's) it joins the same two runs: v ~ v - 1 inside the tile, n ~ n - 1 inside n's tile or by n's own x
            // step in this kernel.  So only the first pair of a run of pairs does the union (induction on tx, which ends at 0); whether
            // a voxel is foreground, and its class, never changes, so the test cannot be stale.
            const bool cross_zy = tz + dz < 0 || ty + dy < 0 || ty + dy >= kCcTY;
            if (cross_zy && left_fg && nx > 0 && joins(n - 1)) continue;
            uf_union<__HIP_MEMORY_SCOPE_AGENT>(parent, v, n);
        }
    }
}

// Streaming pass, four voxels per thread.  parent[] is read-only here (plain loads: a kernel boundary lies between the merge and
// this), labels[] is a separate array.  sizes[]: a tile-local root that is not its component's root moves its count to the root's slot
// with one atomic and clears its own.  Nobody adds to a slot that is not a root, and a root never touches its own slot, so the plain
// accesses and the atomics never meet on one address; integer adds commute, so sizes[] is exact and reproducible.
__global__ __launch_bounds__(kCcThreads) void components_flatten_kernel(const int* __restrict__ parent, long long numel,
        int* __restrict__ labels, int* sizes) {
    const long long quads = numel / 4;
    for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += (long long)gridDim.x * blockDim.x) {
        const int4 p = *reinterpret_cast<const int4*>(parent + 4 * q);
        const int4 c = *reinterpret_cast<const int4*>(sizes + 4 * q);
        const int pv[4] = {p.x, p.y, p.z, p.w}, cv[4] = {c.x, c.y, c.z, c.w};
        int lv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int v = (int)(4 * q + j);
            int rt = pv[j];
            if (rt >= 0 && rt != v) {
                for (;;) {                                  // strictly decreasing (parent[i] <= i)
                    const int up = parent[rt];
                    if (up == rt) break;
                    rt = up;
                }
                if (cv[j] > 0) {
                    atomicAdd(&sizes[rt], cv[j]);
                    sizes[v] = 0;
                }
            }
            lv[j] = rt + 1;                                 // background: -1 + 1 = 0
        }
        *reinterpret_cast<int4*>(labels + 4 * q) = make_int4(lv[0], lv[1], lv[2], lv[3]);
    }
    if (blockIdx.x == 0 && threadIdx.x < (int)(numel - 4 * quads)) {
        const int v = (int)(4 * quads + threadIdx.x);
        int rt = parent[v];
        if (rt >= 0 && rt != v) {
            for (;;) {
                const int up = parent[rt];
                if (up == rt) break;
                rt = up;
            }
            const int c = sizes[v];
            if (c > 0) {
                atomicAdd(&sizes[rt], c);
                sizes[v] = 0;
            }
        }
        labels[v] = rt + 1;
    }
}

__device__ __forceinline__ unsigned long long cc_key(int size, long long slot) {
    // larger size wins, then the smaller label (= slot + 1)
    return size > 0 ? ((unsigned long long)(unsigned)size << 32) | (0xFFFFFFFFull - (unsigned long long)(slot + 1)) : 0ull;
}

// foreground voxels and components are summed, the key takes the maximum: one pass for the three
struct OpCcInfo {
    static __device__ __forceinline__ unsigned long long apply(unsigned long long a, unsigned long long b, int j) {
        return j < 2 ? a + b : (b > a ? b : a);
    }
};

// part[block][3] = foreground voxels, components, max key over this block's share of sizes[]
__global__ __launch_bounds__(kCcThreads) void components_info_kernel(const int* __restrict__ sizes, long long numel,
        unsigned long long* __restrict__ part) {
    unsigned long long acc[3] = {0, 0, 0};      // foreground voxels, components, max key
    const long long quads = numel / 4;
    for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += (long long)gridDim.x * blockDim.x) {
        const int4 c = *reinterpret_cast<const int4*>(sizes + 4 * q);
        const int cv[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            acc[0] += (unsigned)cv[j];
            acc[1] += cv[j] > 0;
            const unsigned long long k = cc_key(cv[j], 4 * q + j);
            acc[2] = k > acc[2] ? k : acc[2];
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < (int)(numel - 4 * quads)) {
        const long long v = 4 * quads + threadIdx.x;
        const int c = sizes[v];
        acc[0] += (unsigned)c;
        acc[1] += c > 0;
        const unsigned long long k = cc_key(c, v);
        acc[2] = k > acc[2] ? k : acc[2];
    }
    block_reduce<OpCcInfo>(acc);
    if (threadIdx.x == 0) for (int j = 0; j < 3; ++j) part[(long long)blockIdx.x * 3 + j] = acc[j];
}

__global__ __launch_bounds__(kCcThreads) void components_info_finalize_kernel(const unsigned long long* __restrict__ part, int nblk,
        int64_t* __restrict__ info) {
    unsigned long long acc[3] = {0, 0, 0};
    partials_reduce<OpCcInfo>(part, nblk, acc);
    block_reduce<OpCcInfo>(acc);
    if (threadIdx.x == 0) {
        const unsigned long long key = acc[2];
        info[0] = (int64_t)acc[0];
        info[1] = (int64_t)acc[1];
        info[2] = (int64_t)(key >> 32);
        info[3] = key ? (int64_t)(0xFFFFFFFFull - (key & 0xFFFFFFFFull)) : 0;
    }
}

// Streaming pass.  mask and out may be the same array (each thread reads its own voxels before it writes them), so neither is
// __restrict__.  keep: n_keep < 0 = no list.  Vec2: both pointers 16-byte aligned, two voxels per load.
__device__ __forceinline__ bool cc_keep(int label, const int* __restrict__ sizes, int min_voxels, const int* keep, int n_keep) {
    if (label == 0) return true;                            // background stays background
    if (sizes[label - 1] < min_voxels) return false;
    if (n_keep < 0) return true;
    bool in = false;
    for (int j = 0; j < n_keep; ++j) in |= keep[j] == label;
    return in;
}

template <bool Vec2>
__global__ __launch_bounds__(kCcThreads) void components_filter_kernel(const int64_t* mask, const int* __restrict__ labels,
        const int* __restrict__ sizes, long long numel, int min_voxels, const int* __restrict__ keep_labels, int n_keep,
        int64_t* out, unsigned long long* __restrict__ removed) {
    __shared__ int keep[16];
    if (threadIdx.x < 16) keep[threadIdx.x] = (int)threadIdx.x < n_keep ? keep_labels[threadIdx.x] : -1;
    __syncthreads();
    long long gone = 0;
    if (Vec2) {
        const long long pairs = numel / 2;
        for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < pairs; q += (long long)gridDim.x * blockDim.x) {
            longlong2 m = *reinterpret_cast<const longlong2*>(mask + 2 * q);
            const int2 l = *reinterpret_cast<const int2*>(labels + 2 * q);
            if (!cc_keep(l.x, sizes, min_voxels, keep, n_keep)) { gone += m.x != 0; m.x = 0; }
            if (!cc_keep(l.y, sizes, min_voxels, keep, n_keep)) { gone += m.y != 0; m.y = 0; }
            *reinterpret_cast<longlong2*>(out + 2 * q) = m;
        }
        if ((numel & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
            int64_t m = mask[numel - 1];
            if (!cc_keep(labels[numel - 1], sizes, min_voxels, keep, n_keep)) { gone += m != 0; m = 0; }
            out[numel - 1] = m;
        }
    } else {
        for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < numel; i += (long long)gridDim.x * blockDim.x) {
            int64_t m = mask[i];
            if (!cc_keep(labels[i], sizes, min_voxels, keep, n_keep)) { gone += m != 0; m = 0; }
            out[i] = m;
        }
    }
    gone = block_reduce_one<OpSum>(gone);
    if (threadIdx.x == 0 && gone) atomicAdd(removed, (unsigned long long)gone);      // one per workgroup; integer, so order-independent
}

// ---- the compact table: rank of a root = the number of roots (sizes[r] > 0) before it in raster order.  Fixed order, no atomics:
// block b of `nblk` owns the contiguous quads [b * chunkq, (b + 1) * chunkq) of sizes[]; rank_count leaves the roots of each chunk,
// rank_scan turns the counts into their exclusive prefix (one block), components_table repeats the walk with a running prefix.
__device__ __forceinline__ int4 cc_load_quad(const int* __restrict__ a, long long q, long long numel) {
    if (4 * q + 4 <= numel) return *reinterpret_cast<const int4*>(a + 4 * q);
    int v[4] = {0, 0, 0, 0};                                // the ragged last quad
    for (int j = 0; j < 4; ++j) if (4 * q + j < numel) v[j] = a[4 * q + j];
    return make_int4(v[0], v[1], v[2], v[3]);
}

// Exclusive prefix sum of one int per thread over the workgroup, in thread order; `total` in every thread.  Every thread calls it.
// A scan, not a reduction (reduce.h has none): shuffles inside a wave, the waves' totals through four LDS slots.
__device__ __forceinline__ int cc_block_exscan(int v, int& total) {
    __shared__ int wsum[kCcWaves];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    int inc = v;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const int up = __shfl_up(inc, o, kWave);
        if (lane >= o) inc += up;
    }
    __syncthreads();                                        // the previous call's reads of wsum are done
    if (lane == kWave - 1) wsum[wave] = inc;
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < kCcWaves; ++w) {
        const int s = wsum[w];
        before += w < wave ? s : 0;
        total += s;
    }
    return before + inc - v;
}

__global__ __launch_bounds__(kCcThreads) void components_rank_count_kernel(const int* __restrict__ sizes, long long numel, long long chunkq,
        int* __restrict__ bcount) {
    const long long quads = (numel + 3) / 4, q0 = blockIdx.x * chunkq, q1 = q0 + chunkq < quads ? q0 + chunkq : quads;
    int roots = 0;
    for (long long q = q0 + threadIdx.x; q < q1; q += kCcThreads) {
        const int4 c = cc_load_quad(sizes, q, numel);
        roots += (c.x > 0) + (c.y > 0) + (c.z > 0) + (c.w > 0);
    }
    roots = block_reduce_one<OpSum>(roots);
    if (threadIdx.x == 0) bcount[blockIdx.x] = roots;
}

// one block: bcount[0..nblk) -> its exclusive prefix, in place, kCcThreads entries per trip with the carry of the trips before
__global__ __launch_bounds__(kCcThreads) void components_rank_scan_kernel(int* __restrict__ bcount, int nblk) {
    int carry = 0;
    for (int base = 0; base < nblk; base += kCcThreads) {   // (uniform trip count: every thread reaches the barriers of the scan)
        const int i = base + threadIdx.x;
        const int v = i < nblk ? bcount[i] : 0;
        int total;
        const int ex = cc_block_exscan(v, total);
        if (i < nblk) bcount[i] = carry + ex;
        carry += total;
    }
}

// first[rank], size[rank], cls[rank] of every root, and lc[root] = rank + 1 -- the ONLY slots of lc[] this kernel writes and the only
// ones components_relabel reads.  `n` bounds the three tables: a root whose rank is not below it writes none of them.
__global__ __launch_bounds__(kCcThreads) void components_table_kernel(const int64_t* __restrict__ mask, const int* __restrict__ sizes,
        long long numel, long long chunkq, const int* __restrict__ boff, int n, int* __restrict__ first, int* __restrict__ size,
        int64_t* __restrict__ cls, int* __restrict__ lc) {
    const long long quads = (numel + 3) / 4, q0 = blockIdx.x * chunkq, q1 = q0 + chunkq < quads ? q0 + chunkq : quads;
    int base = boff[blockIdx.x];
    for (long long qb = q0; qb < q1; qb += kCcThreads) {
        const long long q = qb + threadIdx.x;
        const int4 c = q < q1 ? cc_load_quad(sizes, q, numel) : make_int4(0, 0, 0, 0);
        const int cv[4] = {c.x, c.y, c.z, c.w};
        int total;
        int rank = base + cc_block_exscan((c.x > 0) + (c.y > 0) + (c.z > 0) + (c.w > 0), total);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (cv[j] <= 0) continue;
            const long long v = 4 * q + j;
            if (rank < n) {
                first[rank] = (int)v;
                size[rank] = cv[j];
                cls[rank] = mask[v];
            }
            lc[v] = ++rank;
        }
        base += total;
    }
}

// lc[v] = lc[labels[v] - 1], 0 on background.  The slot of a root is read by every voxel of its component and written by nobody here
// (a root keeps what components_table wrote); every other slot is written once and never read: no race.  A quad without a root is
// one 16-byte store.
__global__ __launch_bounds__(kCcThreads) void components_relabel_kernel(const int* __restrict__ labels, long long numel, int* lc) {
    const long long quads = numel / 4;
    for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += (long long)gridDim.x * blockDim.x) {
        const int4 l = *reinterpret_cast<const int4*>(labels + 4 * q);
        const int lv[4] = {l.x, l.y, l.z, l.w};
        int out[4];
        bool root = false;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool mine = lv[j] - 1 == (int)(4 * q + j);
            root |= mine;
            out[j] = lv[j] <= 0 || lv[j] > numel || mine ? 0 : lc[lv[j] - 1];      // (a label that is none of this volume's: 0)
        }
        if (!root) {
            *reinterpret_cast<int4*>(lc + 4 * q) = make_int4(out[0], out[1], out[2], out[3]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) if (lv[j] - 1 != (int)(4 * q + j)) lc[4 * q + j] = out[j];
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < (int)(numel - 4 * quads)) {
        const long long v = 4 * quads + threadIdx.x;
        const int l = labels[v];
        if (l - 1 != (int)v) lc[v] = l <= 0 || l > numel ? 0 : lc[l - 1];
    }
}

// Streaming pass, the filter by table.  mask and out may be the same array, as in components_filter_kernel.  A label outside 1..n
// (not one of this table's) is treated as not kept rather than read past keep[].
__device__ __forceinline__ bool cc_keep_flag(int l, const unsigned char* __restrict__ keep, int n) {
    return l == 0 || ((unsigned)(l - 1) < (unsigned)n && keep[l - 1] != 0);
}

template <bool Vec2>
__global__ __launch_bounds__(kCcThreads) void components_filter_table_kernel(const int64_t* mask, const int* __restrict__ lc,
        const unsigned char* __restrict__ keep, int n, long long numel, int64_t* out, unsigned long long* __restrict__ removed) {
    long long gone = 0;
    if (Vec2) {
        const long long pairs = numel / 2;
        for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < pairs; q += (long long)gridDim.x * blockDim.x) {
            longlong2 m = *reinterpret_cast<const longlong2*>(mask + 2 * q);
            const int2 l = *reinterpret_cast<const int2*>(lc + 2 * q);
            if (!cc_keep_flag(l.x, keep, n)) { gone += m.x != 0; m.x = 0; }
            if (!cc_keep_flag(l.y, keep, n)) { gone += m.y != 0; m.y = 0; }
            *reinterpret_cast<longlong2*>(out + 2 * q) = m;
        }
        if ((numel & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
            int64_t m = mask[numel - 1];
            if (!cc_keep_flag(lc[numel - 1], keep, n)) { gone += m != 0; m = 0; }
            out[numel - 1] = m;
        }
    } else {
        for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < numel; i += (long long)gridDim.x * blockDim.x) {
            int64_t m = mask[i];
            if (!cc_keep_flag(lc[i], keep, n)) { gone += m != 0; m = 0; }
            out[i] = m;
        }
    }
    gone = block_reduce_one<OpSum>(gone);
    if (threadIdx.x == 0 && gone) atomicAdd(removed, (unsigned long long)gone);      // one per workgroup; integer, so order-independent
}

static size_t cc_parent_bytes(long long numel) { return align_up((size_t)numel * sizeof(int), 256); }
static size_t cc_part_bytes(long long numel) { return align_up((size_t)cc_grid((numel + 3) / 4) * 3 * sizeof(unsigned long long), 256); }
static size_t cc_cvol_bytes(long long numel) { return align_up((size_t)numel, 256); }       // the class volume, 1 byte per voxel
static bool cc_extent_ok(int D, int H, int W) {
    return D > 0 && H > 0 && W > 0 && (long long)D * H <= kCcMaxVoxels && (long long)D * H * W <= kCcMaxVoxels;
}
static size_t cc_ws_bytes(int D, int H, int W, bool classes) {
    if (!cc_extent_ok(D, H, W)) return 0;
    const long long numel = (long long)D * H * W;
    return cc_parent_bytes(numel) + cc_part_bytes(numel) + (classes ? cc_cvol_bytes(numel) : 0);
}
// blocks of the rank passes and the quads of sizes[] each of them owns
static int cc_rank_blocks(long long numel) { return cc_grid((numel + 3) / 4); }
static long long cc_rank_chunk(long long numel) { const int b = cc_rank_blocks(numel); return ((numel + 3) / 4 + b - 1) / b; }

// The labelling call, cut short after its first `steps` launches.  Cls: the class-aware form -- info is int64[8], cleared first
// (the local kernel adds to slot 4, the finalise writes slots 0..3), and the class volume lies behind the partials in the workspace.
template <bool Cls>
static int cc_label_steps(const char* who, const int64_t* mask, int D, int H, int W, int connectivity, int32_t* labels, int32_t* sizes,
                          int64_t* info, void* ws, size_t ws_bytes, int steps, void* stream) {
    SEG_CHECK_ARG(D > 0 && H > 0 && W > 0, "%s: extents must be positive, got %d x %d x %d", who, D, H, W);
    SEG_CHECK_ARG(cc_extent_ok(D, H, W), "%s: %lld voxels; labels are int32, at most 2^31 - 2 voxels", who, (long long)D * H * W);
    SEG_CHECK_ARG(connectivity == 6 || connectivity == 18 || connectivity == 26, "%s: connectivity must be 6, 18 or 26, got %d", who, connectivity);
    SEG_CHECK_WS(cc_ws_bytes(D, H, W, Cls), ws_bytes);
    SEG_CHECK_ARG(mask && labels && sizes && info && ws, "%s: null pointer", who);
    SEG_CHECK_ARG(((uintptr_t)labels | (uintptr_t)sizes | (uintptr_t)ws) % 16 == 0 && (uintptr_t)mask % 8 == 0 &&
                  (!Cls || (uintptr_t)info % 8 == 0),     // (the class-aware form adds to info[4] with a 64-bit atomic)
                  "%s: labels, sizes and the workspace must be 16-byte aligned", who);
    const dim3 tiles(cdiv(W, kCcTX), cdiv(H, kCcTY), cdiv(D, kCcTZ));
    SEG_CHECK_ARG(tiles.y <= 65535u && tiles.z <= 65535u, "%s: more than 65535 tiles along an axis", who);
    hipStream_t st = (hipStream_t)stream;
    const long long numel = (long long)D * H * W;
    ProfScope ps(PF_LOSS, 0.0, (8.0 + 8 + 12 + 4 + (Cls ? 1 : 0)) * numel, st);      // local 8 + 8 (+ 1), flatten 12, info 4 bytes per voxel
    Carver cv(ws);
    int* parent = cv.take<int>((size_t)numel);
    unsigned long long* part = cv.take<unsigned long long>((size_t)cc_grid((numel + 3) / 4) * 3);
    unsigned char* cvol = Cls ? cv.take<unsigned char>((size_t)numel) : nullptr;
    unsigned long long* oob = Cls ? (unsigned long long*)(info + 4) : nullptr;
    if (Cls && hipMemsetAsync(info, 0, 8 * sizeof(int64_t), st) != hipSuccess) { set_error("%s: hipMemsetAsync failed", who); return MI355SEG_EHIP; }
    if (W % 2 == 0 && (uintptr_t)mask % 16 == 0)
        hipLaunchKernelGGL((components_local_kernel<true, Cls>), tiles, dim3(kCcThreads), 0, st, mask, D, H, W, connectivity, parent, sizes, cvol, oob);
    else
        hipLaunchKernelGGL((components_local_kernel<false, Cls>), tiles, dim3(kCcThreads), 0, st, mask, D, H, W, connectivity, parent, sizes, cvol, oob);
    SEG_CHECK_LAUNCH();
    if (steps < 2) return MI355SEG_OK;
    hipLaunchKernelGGL(components_merge_kernel<Cls>, tiles, dim3(kCcThreads), 0, st, parent, (const unsigned char*)cvol, D, H, W, connectivity);
    SEG_CHECK_LAUNCH();
    if (steps < 3) return MI355SEG_OK;
    const int nblk = cc_grid((numel + 3) / 4);
    hipLaunchKernelGGL(components_flatten_kernel, dim3(nblk), dim3(kCcThreads), 0, st, (const int*)parent, numel, labels, sizes);
    SEG_CHECK_LAUNCH();
    if (steps < 4) return MI355SEG_OK;
    hipLaunchKernelGGL(components_info_kernel, dim3(nblk), dim3(kCcThreads), 0, st, (const int*)sizes, numel, part);
    SEG_CHECK_LAUNCH();
    if (steps < 5) return MI355SEG_OK;
    hipLaunchKernelGGL(components_info_finalize_kernel, dim3(1), dim3(kCcThreads), 0, st, (const unsigned long long*)part, nblk, info);
    SEG_CHECK_LAUNCH();
    return MI355SEG_OK;
}

}  // namespace seg

using namespace seg;

extern "C" {

int mi355seg_components_tile_extent(int axis) { return axis == 0 ? kCcTZ : axis == 1 ? kCcTY : axis == 2 ? kCcTX : 0; }

size_t mi355seg_components_ws_bytes(int D, int H, int W) { return cc_ws_bytes(D, H, W, false); }
size_t mi355seg_components_classes_ws_bytes(int D, int H, int W) { return cc_ws_bytes(D, H, W, true); }

int mi355seg_components_label_steps_i64(const int64_t* mask, int D, int H, int W, int connectivity, int32_t* labels, int32_t* sizes, int64_t* info,
                                        void* ws, size_t ws_bytes, int steps, void* stream) {
    SEG_CHECK_ARG(steps >= 1 && steps <= 5, "components_label_steps: steps must lie in 1..5, got %d", steps);
    return cc_label_steps<false>("components_label", mask, D, H, W, connectivity, labels, sizes, info, ws, ws_bytes, steps, stream);
}

int mi355seg_components_label_classes_steps_i64(const int64_t* mask, int D, int H, int W, int connectivity, int32_t* labels, int32_t* sizes,
                                                int64_t* info, void* ws, size_t ws_bytes, int steps, void* stream) {
    SEG_CHECK_ARG(steps >= 1 && steps <= 5, "components_label_classes_steps: steps must lie in 1..5, got %d", steps);
    return cc_label_steps<true>("components_label_classes", mask, D, H, W, connectivity, labels, sizes, info, ws, ws_bytes, steps, stream);
}

int mi355seg_components_label_classes_i64(const int64_t* mask, int D, int H, int W, int connectivity, int32_t* labels, int32_t* sizes,
                                          int64_t* info, void* ws, size_t ws_bytes, void* stream) {
    return cc_label_steps<true>("components_label_classes", mask, D, H, W, connectivity, labels, sizes, info, ws, ws_bytes, 5, stream);
}

int mi355seg_components_label_i64(const int64_t* mask, int D, int H, int W, int connectivity, int32_t* labels, int32_t* sizes, int64_t* info,
                                  void* ws, size_t ws_bytes, void* stream) {
    return mi355seg_components_label_steps_i64(mask, D, H, W, connectivity, labels, sizes, info, ws, ws_bytes, 5, stream);
}

int mi355seg_components_filter_i64(const int64_t* mask, const int32_t* labels, const int32_t* sizes, long long numel, long long min_voxels,
                                   const int32_t* keep_labels, int n_keep, int64_t* out, int64_t* removed, void* stream) {
    SEG_CHECK_ARG(numel > 0 && numel <= kCcMaxVoxels, "components_filter: %lld voxels; between 1 and 2^31 - 2", numel);
    SEG_CHECK_ARG(n_keep >= 0 && n_keep <= 16, "components_filter: the keep list holds 0 to 16 labels, got %d", n_keep);
    SEG_CHECK_ARG(min_voxels >= 0, "components_filter: min_voxels must not be negative, got %lld", min_voxels);
    SEG_CHECK_ARG(mask && labels && sizes && out && removed, "components_filter: null pointer");
    SEG_CHECK_ARG((uintptr_t)labels % 8 == 0, "components_filter: labels must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(PF_LOSS, 0.0, (8.0 + 4 + 8) * numel, st);
    if (hipMemsetAsync(removed, 0, sizeof(int64_t), st) != hipSuccess) { set_error("components_filter: hipMemsetAsync failed"); return MI355SEG_EHIP; }
    const int mv = (int)(min_voxels > kCcMaxVoxels + 1 ? kCcMaxVoxels + 1 : min_voxels);    // no component is larger than numel
    const int nk = keep_labels ? n_keep : -1;
    if (((uintptr_t)mask | (uintptr_t)out) % 16 == 0)
        hipLaunchKernelGGL(components_filter_kernel<true>, dim3(cc_grid((numel + 1) / 2)), dim3(kCcThreads), 0, st, mask, labels, sizes, numel, mv,
                           keep_labels, nk, out, (unsigned long long*)removed);
    else
        hipLaunchKernelGGL(components_filter_kernel<false>, dim3(cc_grid(numel)), dim3(kCcThreads), 0, st, mask, labels, sizes, numel, mv,
                           keep_labels, nk, out, (unsigned long long*)removed);
    SEG_CHECK_LAUNCH();
    return MI355SEG_OK;
}

size_t mi355seg_components_table_ws_bytes(long long numel) {
    return numel > 0 && numel <= kCcMaxVoxels ? align_up((size_t)cc_rank_blocks(numel) * sizeof(int), 256) : 0;
}

int mi355seg_components_table_i64(const int64_t* mask, const int32_t* labels, const int32_t* sizes, long long numel, long long n,
                                  int32_t* labels_consecutive, int32_t* first, int32_t* size, int64_t* cls,
                                  void* ws, size_t ws_bytes, void* stream) {
    SEG_CHECK_ARG(numel > 0 && numel <= kCcMaxVoxels, "components_table: %lld voxels; between 1 and 2^31 - 2", numel);
    SEG_CHECK_ARG(n >= 0 && n <= numel, "components_table: n = %lld components; between 0 and the %lld voxels", n, numel);
    SEG_CHECK_WS(mi355seg_components_table_ws_bytes(numel), ws_bytes);
    SEG_CHECK_ARG(mask && labels && sizes && labels_consecutive && ws, "components_table: null pointer");
    SEG_CHECK_ARG(n == 0 || (first && size && cls), "components_table: null table with n = %lld", n);
    SEG_CHECK_ARG(((uintptr_t)labels | (uintptr_t)sizes | (uintptr_t)labels_consecutive | (uintptr_t)ws) % 16 == 0 && (uintptr_t)mask % 8 == 0 &&
                  ((uintptr_t)first | (uintptr_t)size) % 4 == 0 && (uintptr_t)cls % 8 == 0,
                  "components_table: labels, sizes, labels_consecutive and the workspace must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(PF_LOSS, 0.0, (4.0 + 4 + 4 + 4) * numel, st);       // count 4, table 4, relabel 4 + 4 bytes per voxel
    const int nblk = cc_rank_blocks(numel);
    const long long chunkq = cc_rank_chunk(numel);
    int* bcount = (int*)ws;
    hipLaunchKernelGGL(components_rank_count_kernel, dim3(nblk), dim3(kCcThreads), 0, st, sizes, numel, chunkq, bcount);
    SEG_CHECK_LAUNCH();
    hipLaunchKernelGGL(components_rank_scan_kernel, dim3(1), dim3(kCcThreads), 0, st, bcount, nblk);
    SEG_CHECK_LAUNCH();
    hipLaunchKernelGGL(components_table_kernel, dim3(nblk), dim3(kCcThreads), 0, st, mask, sizes, numel, chunkq, (const int*)bcount, (int)n,
                       first, size, cls, labels_consecutive);
    SEG_CHECK_LAUNCH();
    hipLaunchKernelGGL(components_relabel_kernel, dim3(cc_grid((numel + 3) / 4)), dim3(kCcThreads), 0, st, labels, numel, labels_consecutive);
    SEG_CHECK_LAUNCH();
    return MI355SEG_OK;
}

int mi355seg_components_filter_table_i64(const int64_t* mask, const int32_t* labels_consecutive, const uint8_t* keep, long long n,
                                         long long numel, int64_t* out, int64_t* removed, void* stream) {
    SEG_CHECK_ARG(numel > 0 && numel <= kCcMaxVoxels, "components_filter_table: %lld voxels; between 1 and 2^31 - 2", numel);
    SEG_CHECK_ARG(n >= 0 && n <= numel, "components_filter_table: n = %lld keep flags; between 0 and the %lld voxels", n, numel);
    SEG_CHECK_ARG(mask && labels_consecutive && out && removed, "components_filter_table: null pointer");
    SEG_CHECK_ARG(n == 0 || keep, "components_filter_table: null keep flags with n = %lld", n);
    SEG_CHECK_ARG((uintptr_t)labels_consecutive % 8 == 0 && ((uintptr_t)mask | (uintptr_t)out | (uintptr_t)removed) % 8 == 0,
                  "components_filter_table: labels_consecutive must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(PF_LOSS, 0.0, (8.0 + 4 + 8) * numel, st);
    if (hipMemsetAsync(removed, 0, sizeof(int64_t), st) != hipSuccess) { set_error("components_filter_table: hipMemsetAsync failed"); return MI355SEG_EHIP; }
    if (((uintptr_t)mask | (uintptr_t)out) % 16 == 0)
        hipLaunchKernelGGL(components_filter_table_kernel<true>, dim3(cc_grid((numel + 1) / 2)), dim3(kCcThreads), 0, st, mask, labels_consecutive,
                           keep, (int)n, numel, out, (unsigned long long*)removed);
    else
        hipLaunchKernelGGL(components_filter_table_kernel<false>, dim3(cc_grid(numel)), dim3(kCcThreads), 0, st, mask, labels_consecutive,
                           keep, (int)n, numel, out, (unsigned long long*)removed);
    SEG_CHECK_LAUNCH();
    return MI355SEG_OK;
}

}  // extern "C"
