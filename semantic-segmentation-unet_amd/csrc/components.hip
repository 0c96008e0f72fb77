// Connected components of a batch of class maps, with the canonical numbering, a minimum-area filter and an integer object table.
//   connected  = 4- or 8-neighbours of one image carrying the same class, that class not `background`
//   labels     = 0 on background, else 1 + the rank of the component among its image's components ordered by the row-major index of each
//                component's first pixel; count[n] = components of image n; a function of the mask alone
//   filter     = components below min_area pixels become background in mask_out and 0 in labels; survivors keep their order, renumbered
//   objects    = int64 [N, max_objects, 8], row label - 1: class, area, y0, x0, y1, x1 (inclusive), sum y, sum x
// Label equivalence by union-find over the linear pixel index p = (n H + y) W + x, the SMALLER index the parent, so a component's root is
// its first pixel in row-major order.  par[p] = -1 on background, else an index <= p of the same component.  Launches, in order:
//   1. local_kernel    one workgroup per 32 x 64 tile: union-find of the tile in LDS (left / up / up-left / up-right links), flattened, written
//                      to par as global indices (tile-local row-major order is global row-major order, so the tile root is the tile's first
//                      pixel of the component); zeroes area
//   2. border_kernel   a lane per pixel of a tile's top row, left and right column: links to the backward neighbours that lie in ANOTHER tile.
//                      par is shared by every workgroup of this launch: read with agent-scope atomic loads, linked with atomicMin only
//   3. flatten_kernel  par[p] = root of p (no links are made here: the roots are fixed, every writer of a word writes its root)
//   4. area_kernel     area[root] += pixels, only when min_area > 1
//   5. count_kernel / scan_kernel / apply_kernel   the three-launch exclusive scan over the kept roots (root and area >= min_area) in row-major
//                      order, per image: per-block counts, ONE block per image scans that image's counts (and writes count_out), every block redoes its own scan
//                      and writes the new label over area[root] (0 for a removed root).  Roots are first pixels: this is the canonical numbering
//   6. table_init_kernel  rows < min(count, max_objects) of the table: area 0, an empty box, sums 0
//   7. relabel_kernel  labels_out = area[par[p]], mask_out, and the table by integer atomic add / min / max
// Termination, no loop depends on another workgroup's progress: every word of par (and of the LDS array) only ever DEcreases and par[a] <= a.
// find(a) follows a strictly decreasing chain of indices >= 0, so it ends, whatever other lanes store meanwhile.  A stale read returns a value
// the word held earlier: still an index <= a of the same component, so the chain stays inside the component and stays decreasing.  union(a, b):
// a = find(a), b = find(b); equal: done; else with a > b, old = atomicMin(par + a, b); old == a: a was a root at that instant and now hangs below
// b: done; else a was no root any more (another lane linked it, or the read that called it a root was stale): par[a] = min(old, b), both of the
// component, and the loop goes on with union(old, b), which keeps the link a - old that the minimum may have replaced.  The pair's maximum strictly
// decreases (old < a, b < a), so the loop ends after at most a trips.  Nothing waits, nothing spins on a flag.
// Ordering: the only atomics are minimum-index links, integer adds and integer min / max; none of their results depends on arrival order (the
// set of links made differs from run to run, the partition and so the flattened roots do not).  No floating point anywhere: the same bits run
// after run.  Runs of equal key are pre-reduced per wave (and across the 16 rows of pixels a wave visits) before any global atomic: one component
// covering the image costs one atomic set per 1024 pixels, not one per pixel.
#include "common.h"

namespace {

constexpr int WG = 256;
constexpr int TH = 32, TW = 64, TPIX = TH * TW;      // tile of the LDS pass; TW = one wave: a wave's stores are one tile row
constexpr int BORDER = TW + 2 * TH;                  // border lanes per tile: top row, left column, right column
constexpr int SCAN_PER = 8, SCAN_CH = WG * SCAN_PER; // pixels per lane / per block of the scan kernels (consecutive per lane: row-major ranks)
constexpr int RL_ITER = 16, RL_CH = WG * RL_ITER;    // rows of 256 pixels per block of the area and relabel kernels

__device__ __forceinline__ int mask_at(const void* m, int elem, long off) {
    return elem == 1 ? (int)reinterpret_cast<const uint8_t*>(m)[off] : reinterpret_cast<const int*>(m)[off];
}

// ---- LDS union-find (one workgroup) ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int lds_find(volatile int* L, int a) {
    int p;
    while ((p = L[a]) != a) a = p;                   // L[a] <= a: strictly decreasing
    return a;
}
__device__ __forceinline__ void lds_union(int* L, int a, int b) {
    for (;;) {
        a = lds_find(L, a); b = lds_find(L, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&L[a], b);
        if (old == a) return;
        a = old;                                     // old < a: the maximum of the pair decreases
    }
}

__global__ __launch_bounds__(WG) void local_kernel(const void* __restrict__ mask, int elem, long pitch, int H, int W, int tilesY, int tilesX,
                                                   int conn8, int background, int* __restrict__ par, int* __restrict__ area) {
    __shared__ int L[TPIX];
    __shared__ int C[TPIX];
    __shared__ unsigned char F[TPIX];
    const int tx = blockIdx.x % tilesX, r0 = blockIdx.x / tilesX, ty = r0 % tilesY, n = r0 / tilesY;
    const int y0 = ty * TH, x0 = tx * TW;
    for (int i = threadIdx.x; i < TPIX; i += WG) {
        const int y = y0 + (i >> 6), x = x0 + (i & 63);
        const bool in = y < H && x < W;
        const int c = in ? mask_at(mask, elem, ((long)n * H + y) * pitch + x) : 0;
        C[i] = c; F[i] = in && (background < 0 || c != background); L[i] = i;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < TPIX; i += WG) {
        if (!F[i]) continue;
        const int c = C[i], ly = i >> 6, lx = i & 63;
        if (lx > 0 && F[i - 1] && C[i - 1] == c) lds_union(L, i, i - 1);
        if (ly > 0) {
            if (F[i - TW] && C[i - TW] == c) lds_union(L, i, i - TW);       // (8-connectivity: the row links of `up` reach both diagonals)
            else if (conn8) {
                if (lx > 0 && F[i - TW - 1] && C[i - TW - 1] == c) lds_union(L, i, i - TW - 1);
                if (lx < TW - 1 && F[i - TW + 1] && C[i - TW + 1] == c) lds_union(L, i, i - TW + 1);
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < TPIX; i += WG) {
        const int y = y0 + (i >> 6), x = x0 + (i & 63);
        if (y >= H || x >= W) continue;
        const int g = (n * H + y) * W + x;
        int v = -1;
        if (F[i]) { const int r = lds_find(L, i); v = (n * H + y0 + (r >> 6)) * W + x0 + (r & 63); }
        par[g] = v; area[g] = 0;
    }
}

// ---- global union-find: par is shared by the workgroups of one launch ----------------------------------------------------------------------
__device__ __forceinline__ int ld_agent(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int g_find(const int* par, int a) {
    for (;;) { const int p = ld_agent(par + a); if (p == a) return a; a = p; }      // p < a
}
__device__ __forceinline__ void g_union(int* par, int a, int b) {
    for (;;) {
        a = g_find(par, a); b = g_find(par, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(par + a, b);
        if (old == a) return;
        a = old;
    }
}

__global__ __launch_bounds__(WG) void border_kernel(const void* __restrict__ mask, int elem, long pitch, int H, int W, int tilesY, int tilesX,
                                                    long ntiles, int conn8, int background, int* par) {
    const long gid = (long)blockIdx.x * WG + threadIdx.x;
    const long tile = gid / BORDER;
    const int k = (int)(gid % BORDER);
    if (tile >= ntiles || (!conn8 && k >= TW + TH)) return;
    const int tx = (int)(tile % tilesX); const long r0 = tile / tilesX;
    const int ty = (int)(r0 % tilesY), n = (int)(r0 / tilesY);
    const int ly = k < TW ? 0 : (k < TW + TH ? k - TW : k - TW - TH), lx = k < TW ? k : (k < TW + TH ? 0 : TW - 1);
    const int y = ty * TH + ly, x = tx * TW + lx;
    if (y >= H || x >= W) return;
    const long row = (long)n * H + y;
    const int c = mask_at(mask, elem, row * pitch + x);
    if (background >= 0 && c == background) return;
    const int p = (int)(row * W + x);
    auto link = [&](int yy, int xx) {
        if (yy < 0 || xx < 0 || xx >= W) return;
        if (yy / TH == ty && xx / TW == tx) return;                          // the LDS pass made this link
        if (mask_at(mask, elem, ((long)n * H + yy) * pitch + xx) == c) g_union(par, p, (n * H + yy) * W + xx);
    };
    link(y, x - 1); link(y - 1, x);
    if (conn8) { link(y - 1, x - 1); link(y - 1, x + 1); }
}

__global__ __launch_bounds__(WG) void flatten_kernel(int* par, long P) {
    const long p = (long)blockIdx.x * WG + threadIdx.x;
    if (p >= P) return;
    const int v = ld_agent(par + p);
    if (v < 0 || v == (int)p) return;
    const int r = g_find(par, v);
    if (r != v) atomicMin(par + v, r);                                       // the tile root, shared by the tile's pixels of this component
    __hip_atomic_store(par + p, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- per-wave reduction of runs of equal key before the global atomics ---------------------------------------------------------------------
template <bool FULL> struct Stat { int cnt, y0, y1, x0, x1; long long sy, sx; };
template <bool FULL> __device__ __forceinline__ void combine(Stat<FULL>& a, const Stat<FULL>& b) {
    a.cnt += b.cnt;
    if constexpr (FULL) {
        a.y0 = min(a.y0, b.y0); a.y1 = max(a.y1, b.y1); a.x0 = min(a.x0, b.x0); a.x1 = max(a.x1, b.x1); a.sy += b.sy; a.sx += b.sx;
    }
}
template <bool FULL> __device__ __forceinline__ Stat<FULL> shfl_down_stat(const Stat<FULL>& s, int d) {
    Stat<FULL> o = s;
    o.cnt = __shfl_down(s.cnt, d);
    if constexpr (FULL) {
        o.y0 = __shfl_down(s.y0, d); o.y1 = __shfl_down(s.y1, d); o.x0 = __shfl_down(s.x0, d); o.x1 = __shfl_down(s.x1, d);
        o.sy = __shfl_down(s.sy, d); o.sx = __shfl_down(s.sx, d);
    }
    return o;
}
// Every lane of the wave calls this (key < 0: the lane holds nothing).  acc_key / acc are wave-uniform: the sum of the whole-wave runs seen so far
// of one key, handed to emit by lane 0 when another key arrives.  A wave that holds several runs reduces each to its first lane, which emits it.
// The coordinate sums are 64-bit: a one-column image may be 2^31 - 1 rows tall.
template <bool FULL, class Emit>
__device__ __forceinline__ void wave_runs(int key, Stat<FULL> s, int& acc_key, Stat<FULL>& acc, Emit emit) {
    const int lane = threadIdx.x & 63;
    const int prev = __shfl_up(key, 1);
    const bool head = lane == 0 || prev != key;
    const unsigned long long hm = __ballot(head);
    const unsigned long long rest = lane == 63 ? 0ull : hm >> (lane + 1);
    const int runend = rest ? lane + __ffsll((long long)rest) - 1 : 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const Stat<FULL> o = shfl_down_stat(s, d);
        if (lane + d <= runend) combine(s, o);
    }
    if (hm == 1ull && key >= 0) {                                            // (wave-uniform) one run fills the wave; lane 0 holds its sum
        Stat<FULL> whole = s;
        whole.cnt = __shfl(s.cnt, 0);
        if constexpr (FULL) {
            whole.y0 = __shfl(s.y0, 0); whole.y1 = __shfl(s.y1, 0); whole.x0 = __shfl(s.x0, 0); whole.x1 = __shfl(s.x1, 0);
            whole.sy = __shfl(s.sy, 0); whole.sx = __shfl(s.sx, 0);
        }
        if (key == acc_key) { combine(acc, whole); return; }
        if (acc_key >= 0 && lane == 0) emit(acc_key, acc);
        acc_key = key; acc = whole;
        return;
    }
    if (acc_key >= 0 && lane == 0) emit(acc_key, acc);
    acc_key = -1;
    if (head && key >= 0) emit(key, s);
}

__global__ __launch_bounds__(WG) void area_kernel(const int* __restrict__ par, int* __restrict__ area, int HW, int bpi) {
    const int n = blockIdx.x / bpi, base = (blockIdx.x % bpi) * RL_CH;
    int acc_key = -1;
    Stat<false> acc = {};
    auto emit = [&](int key, const Stat<false>& s) { atomicAdd(area + key, s.cnt); };
    for (int j = 0; j < RL_ITER; ++j) {
        const int q = base + j * WG + (int)threadIdx.x;
        if (base + j * WG >= HW) break;                                      // (block-uniform)
        int key = -1;
        Stat<false> s = {};
        if (q < HW) { key = par[(long)n * HW + q]; s.cnt = 1; }
        wave_runs<false>(key, s, acc_key, acc, emit);
    }
    if (acc_key >= 0 && (threadIdx.x & 63) == 0) emit(acc_key, acc);
}

// ---- the three-launch scan over the kept roots --------------------------------------------------------------------------------------------
// exclusive scan of one int per lane over the workgroup; *total = the sum
__device__ __forceinline__ int block_excl_scan(int v, int* total) {
    __shared__ int wsum[WG / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(inc, d); if (lane >= d) inc += t; }
    __syncthreads();                                                         // (a previous call's readers of wsum are done)
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int off = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < WG / 64; ++w) { const int t = wsum[w]; if (w < wave) off += t; tot += t; }
    *total = tot;
    return off + inc - v;
}
__device__ __forceinline__ bool kept(const int* par, const int* area, long p, int min_area) {
    return par[p] == (int)p && (min_area <= 1 || area[p] >= min_area);
}

__global__ __launch_bounds__(WG) void count_kernel(const int* __restrict__ par, const int* __restrict__ area, int HW, int bps, int min_area,
                                                   int* __restrict__ blockcnt) {
    const int n = blockIdx.x / bps, base = (blockIdx.x % bps) * SCAN_CH + (int)threadIdx.x * SCAN_PER;
    int c = 0;
    for (int k = 0; k < SCAN_PER; ++k)
        if (base + k < HW) c += kept(par, area, (long)n * HW + base + k, min_area);
    int total;
    block_excl_scan(c, &total);
    if (threadIdx.x == 0) blockcnt[blockIdx.x] = total;
}

// One workgroup per image (images of one block: a lane per image).  blockoff = exclusive scan of blockcnt within the image;
// count_out[n] = the image's total.  No workgroup reads what another one writes.
__global__ __launch_bounds__(WG) void scan_kernel(const int* __restrict__ blockcnt, int* __restrict__ blockoff, int* __restrict__ count_out, int N, int bps) {
    if (bps == 1) {
        const long n = (long)blockIdx.x * WG + threadIdx.x;
        if (n < N) { blockoff[n] = 0; count_out[n] = blockcnt[n]; }
        return;
    }
    const int n = blockIdx.x;
    int carry = 0;
    for (int b0 = 0; b0 < bps; b0 += WG) {
        const int i = b0 + (int)threadIdx.x;
        const int v = i < bps ? blockcnt[(long)n * bps + i] : 0;
        int total;
        const int e = block_excl_scan(v, &total);
        if (i < bps) blockoff[(long)n * bps + i] = carry + e;
        carry += total;
    }
    if (threadIdx.x == 0) count_out[n] = carry;
}

// area[root] := the root's new label (1-based rank among its image's kept roots), 0 for a removed root
__global__ __launch_bounds__(WG) void apply_kernel(const int* __restrict__ par, int* __restrict__ area, int HW, int bps, int min_area,
                                                   const int* __restrict__ blockoff) {
    const int n = blockIdx.x / bps, base = (blockIdx.x % bps) * SCAN_CH + (int)threadIdx.x * SCAN_PER;
    bool f[SCAN_PER];
    int c = 0;
#pragma unroll
    for (int k = 0; k < SCAN_PER; ++k) { f[k] = base + k < HW && kept(par, area, (long)n * HW + base + k, min_area); c += f[k]; }
    int total;
    int label = blockoff[blockIdx.x] + block_excl_scan(c, &total);
#pragma unroll
    for (int k = 0; k < SCAN_PER; ++k) {
        if (base + k >= HW) continue;
        const long p = (long)n * HW + base + k;
        if (par[p] == (int)p) area[p] = f[k] ? ++label : 0;
    }
}

// ---- the object table and the relabelling --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WG) void table_init_kernel(const int* __restrict__ count, long long* __restrict__ objects, int N, int max_objects, int H, int W) {
    const long total = (long)N * max_objects, stride = (long)gridDim.x * WG;
    for (long t = (long)blockIdx.x * WG + threadIdx.x; t < total; t += stride) {
        const int n = (int)(t / max_objects), i = (int)(t % max_objects);
        if (i >= count[n]) continue;
        long long* row = objects + t * 8;
        row[0] = 0; row[1] = 0; row[2] = H; row[3] = W; row[4] = -1; row[5] = -1; row[6] = 0; row[7] = 0;
    }
}

__global__ __launch_bounds__(WG) void relabel_kernel(const void* mask, int elem, long pitch, int H, int W, int HW, int bpi, int background,
                                                     const int* __restrict__ par, const int* __restrict__ newlabel, int* __restrict__ labels,
                                                     void* mask_out, long long* objects, int max_objects) {
    const int n = blockIdx.x / bpi, base = (blockIdx.x % bpi) * RL_CH;
    int acc_key = -1;
    Stat<true> acc = {};
    long long* table = objects ? objects + (long)n * max_objects * 8 : nullptr;
    auto emit = [&](int key, const Stat<true>& s) {
        long long* row = table + (long)(key - 1) * 8;
        __hip_atomic_fetch_add(row + 1, (long long)s.cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_min(row + 2, (long long)s.y0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_min(row + 3, (long long)s.x0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_max(row + 4, (long long)s.y1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_max(row + 5, (long long)s.x1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(row + 6, s.sy, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(row + 7, s.sx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    for (int j = 0; j < RL_ITER; ++j) {
        const int q = base + j * WG + (int)threadIdx.x;
        if (base + j * WG >= HW) break;                                      // (block-uniform)
        int key = -1;
        Stat<true> s = {};
        if (q < HW) {
            const long p = (long)n * HW + q;
            const int r = par[p];
            const int lab = r < 0 ? 0 : newlabel[r];
            labels[p] = lab;
            const int y = q / W, x = q - y * W;
            if (mask_out || table) {
                const int c = mask_at(mask, elem, ((long)n * H + y) * pitch + x);
                if (mask_out) {
                    const int o = (r >= 0 && lab == 0) ? background : c;
                    if (elem == 1) reinterpret_cast<uint8_t*>(mask_out)[p] = (uint8_t)o; else reinterpret_cast<int*>(mask_out)[p] = o;
                }
                if (table && lab > 0 && lab <= max_objects) {
                    key = lab;
                    s.cnt = 1; s.y0 = s.y1 = s.sy = y; s.x0 = s.x1 = s.sx = x;
                    // the class: one writer per row, the component's first pixel (an atomic store: the row's other words take atomics)
                    if (r == (int)p) __hip_atomic_store(table + (long)(lab - 1) * 8, (long long)c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
        }
        if (table) wave_runs<true>(key, s, acc_key, acc, emit);
    }
    if (table && acc_key >= 0 && (threadIdx.x & 63) == 0) emit(acc_key, acc);
}

struct Layout { size_t par, area, cnt, off, bytes; int bps, bpi, tilesY, tilesX; };
size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }
bool shape_ok(int N, int H, int W) { return N >= 1 && H >= 1 && W >= 1 && (long)N * H * W < 0x80000000L; }
Layout layout_of(int N, int H, int W) {
    Layout l;
    const size_t P = (size_t)N * H * W;
    const long HW = (long)H * W;
    l.bps = (int)((HW + SCAN_CH - 1) / SCAN_CH);
    l.bpi = (int)((HW + RL_CH - 1) / RL_CH);
    l.tilesY = (H + TH - 1) / TH; l.tilesX = (W + TW - 1) / TW;
    l.par = 0;
    l.area = align16(P * 4);
    l.cnt = l.area + align16(P * 4);
    l.off = l.cnt + align16((size_t)N * l.bps * 4);
    l.bytes = l.off + align16((size_t)N * l.bps * 4);
    return l;
}
bool overlaps(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
    return a && b && na && nb && pa < pb + nb && pb < pa + na;
}

}  // namespace

extern "C" size_t unet_label_components_workspace(int N, int H, int W) {
    if (!shape_ok(N, H, W)) return 0;
    const Layout l = layout_of(N, H, W);
    // every grid below is one-dimensional: tiles and blocks per image times N stay below 2^31 because N H W does
    return l.bytes;
}

extern "C" int unet_label_components(const void* mask, int mask_elem, long mask_pitch, int N, int H, int W, int connectivity, int background,
                                     int min_area, int* labels_out, int* count_out, void* mask_out, long long* objects_out, int max_objects,
                                     void* ws, size_t ws_bytes, void* stream) {
    UNET_CHECK_ARG(connectivity == 4 || connectivity == 8);
    UNET_CHECK_ARG(mask_elem == 1 || mask_elem == 4);
    UNET_CHECK_ARG(shape_ok(N, H, W) && mask_pitch >= W);
    UNET_CHECK_ARG(background >= -1 && (mask_elem == 4 || background <= 255));
    UNET_CHECK_ARG(min_area >= 0 && !(min_area > 0 && background < 0));
    UNET_CHECK_ARG(!(objects_out && max_objects < 1));
    UNET_CHECK_ARG(mask && labels_out && count_out && ws);
    UNET_CHECK_ARG((reinterpret_cast<uintptr_t>(ws) & 15u) == 0);
    UNET_CHECK_ARG((reinterpret_cast<uintptr_t>(labels_out) & 3u) == 0 && (reinterpret_cast<uintptr_t>(count_out) & 3u) == 0);
    UNET_CHECK_ARG((reinterpret_cast<uintptr_t>(objects_out) & 7u) == 0);
    UNET_CHECK_ARG(mask_elem == 1 || ((reinterpret_cast<uintptr_t>(mask) & 3u) == 0 && (reinterpret_cast<uintptr_t>(mask_out) & 3u) == 0));
    const Layout l = layout_of(N, H, W);
    if (ws_bytes < l.bytes) return UNET_ENOSPC;
    const size_t P = (size_t)N * H * W;
    const size_t in_bytes = (((size_t)N * H - 1) * (size_t)mask_pitch + W) * mask_elem;
    const size_t obj_bytes = objects_out ? (size_t)N * max_objects * 64 : 0;
    {   // nothing written may lie over the input or over another output; mask_out == mask is the one alias, for dense rows
        const void* out[5] = {labels_out, count_out, mask_out, objects_out, ws};
        const size_t nb[5] = {P * 4, (size_t)N * 4, mask_out ? P * mask_elem : 0, obj_bytes, l.bytes};
        for (int i = 0; i < 5; ++i) {
            const bool alias = i == 2 && mask_out == mask && mask_pitch == W;
            UNET_CHECK_ARG(alias || !overlaps(mask, in_bytes, out[i], nb[i]));
            for (int j = i + 1; j < 5; ++j) UNET_CHECK_ARG(!overlaps(out[i], nb[i], out[j], nb[j]));
        }
    }
    hipStream_t st = (hipStream_t)stream;
    int* par = reinterpret_cast<int*>((char*)ws + l.par);
    int* area = reinterpret_cast<int*>((char*)ws + l.area);
    int* blockcnt = reinterpret_cast<int*>((char*)ws + l.cnt);
    int* blockoff = reinterpret_cast<int*>((char*)ws + l.off);
    const int conn8 = connectivity == 8, HW = H * W;
    const long ntiles = (long)N * l.tilesY * l.tilesX;
    local_kernel<<<(unsigned)ntiles, WG, 0, st>>>(mask, mask_elem, mask_pitch, H, W, l.tilesY, l.tilesX, conn8, background, par, area);
    int rc = UNET_LAUNCH_STATUS(); if (rc) return rc;
    if (ntiles > N) {                                                        // (one tile per image: nothing crosses a tile border)
        border_kernel<<<(unsigned)((ntiles * BORDER + WG - 1) / WG), WG, 0, st>>>(mask, mask_elem, mask_pitch, H, W, l.tilesY, l.tilesX, ntiles,
                                                                                  conn8, background, par);
        rc = UNET_LAUNCH_STATUS(); if (rc) return rc;
        flatten_kernel<<<(unsigned)((P + WG - 1) / WG), WG, 0, st>>>(par, (long)P);
        rc = UNET_LAUNCH_STATUS(); if (rc) return rc;
    }
    if (min_area > 1) {
        area_kernel<<<N * l.bpi, WG, 0, st>>>(par, area, HW, l.bpi);
        rc = UNET_LAUNCH_STATUS(); if (rc) return rc;
    }
    count_kernel<<<N * l.bps, WG, 0, st>>>(par, area, HW, l.bps, min_area, blockcnt);
    rc = UNET_LAUNCH_STATUS(); if (rc) return rc;
    scan_kernel<<<l.bps == 1 ? (N + WG - 1) / WG : N, WG, 0, st>>>(blockcnt, blockoff, count_out, N, l.bps);
    rc = UNET_LAUNCH_STATUS(); if (rc) return rc;
    apply_kernel<<<N * l.bps, WG, 0, st>>>(par, area, HW, l.bps, min_area, blockoff);
    rc = UNET_LAUNCH_STATUS(); if (rc) return rc;
    if (objects_out) {
        long nb = ((long)N * max_objects + WG - 1) / WG; if (nb > 65536) nb = 65536;
        table_init_kernel<<<(unsigned)nb, WG, 0, st>>>(count_out, objects_out, N, max_objects, H, W);
        rc = UNET_LAUNCH_STATUS(); if (rc) return rc;
    }
    relabel_kernel<<<N * l.bpi, WG, 0, st>>>(mask, mask_elem, mask_pitch, H, W, HW, l.bpi, background, par, area, labels_out, mask_out,
                                             objects_out, max_objects);
    return UNET_LAUNCH_STATUS();
}
