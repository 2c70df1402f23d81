// K24: SLIC's connectivity pass (data_preparation/superpixel_segmenter_dsec_slic.py:19-24 of the reference calls
//   skimage.segmentation.slic with its default enforce_connectivity=True): every 4-connected component of equal labels smaller
//   than min_size is absorbed into a neighbour, the others are renumbered 0 .. n - 1 in raster order of their first pixel.
//   One deliberate difference: skimage cuts its flood fill at max_size pixels, which depends on the fill order; here a
//   component of any size stays whole.
// The order-free form of skimage's sequential loop (DESIGN.md K24 "Connectivity"): a component's ROOT is its lowest raster
//   index; a component is KEPT iff its size >= min_size and its label is its rank among the kept roots; a small component walks
//   its pixels breadth first from its root (neighbours right, left, down, up) and takes the final label of its DONOR, the last
//   neighbour pixel seen that lies in a component with a smaller root, or 0 when it sees none.
// Five phases, nine launches, all B samples in each, int32 planes of the workspace indexed by the pixel's raster index in its
// sample, integer atomics only (the result is a function of the input partition: it repeats bit for bit), no wait on another
// workgroup anywhere, and every loop bounded by the data:
//   1 components  cc_init, cc_merge (union-find, roots joined with atomicMin so the root is the lowest index whatever the order;
//                 parent[p] <= p always, so a chase strictly decreases), cc_flatten (parent = root)
//   2 sizes       in cc_flatten: atomicAdd at the root, one per run of equal roots in a wave
//   3 ranks       cc_count (kept roots per 256-pixel chunk), cc_scan (one workgroup per sample), cc_rank
//   4 donors      cc_donor: ONE LANE per small root walks its component through a queue segment of the global queue plane,
//                 reserved with one atomicAdd of its size on the sample's cursor (the offsets differ from run to run and touch
//                 no result); bounded by the size of phase 2.  Divergent and latency bound by design.
//   5 resolve     cc_resolve follows each root's donor chain (the roots strictly decrease) into the size plane, which is
//                 dead by then; cc_write stores final(root(pixel)) as int64.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include "oess.h"
#include "oess_common.h"

namespace {
using namespace oess;

typedef unsigned long long u64_t;

constexpr int CC_THREADS = 256;                   // one pixel per thread; a workgroup owns a chunk of 256 consecutive pixels of one sample
constexpr int CC_MAX_PIXELS = 1 << 24;
constexpr int CC_PLANES = 5;                      // parent, size, fin, queue, visited
constexpr int CC_NO_DONOR = INT_MIN;              // fin of a small root: -1 - donor's root, or this
constexpr int CC_PHASES = 5;
#if defined(__HIP_DEVICE_COMPILE__) && defined(__AMDGCN_WAVEFRONT_SIZE) && __AMDGCN_WAVEFRONT_SIZE != 64
#error "the run counts of cc_flatten and the prefix of cc_rank need 64-lane waves"
#endif

struct Planes {
    int *parent, *size, *fin, *queue, *visited;   // [B][HW] each
    int *chunks;                                  // [B][nchunk] kept roots per chunk, then their exclusive prefix
    int *cursor;                                  // [B] next free slot of the sample's queue plane
};

__device__ __forceinline__ int cc_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// parent[q] <= q for every q at every time: the chase strictly decreases and ends at a q with parent[q] == q
__device__ __forceinline__ int cc_find(const int* parent, int p) {
    for (int q; (q = cc_load(parent + p)) < p;) p = q;
    return p;
}

// Joins the sets of a and b.  A parent only ever decreases (atomicMin), so a root read here may have stopped being one: the
// atomicMin then returns what it became and the join goes on from there.  max(a, b) strictly decreases per turn.
__device__ __forceinline__ void cc_unite(int* parent, int a, int b) {
    for (;;) {
        a = cc_find(parent, a);
        b = cc_find(parent, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(parent + a, b);
        if (old == a) return;
        a = old;                                   // old < a: a had been joined elsewhere in between
    }
}

#define CC_PIXEL                                                                  \
    const int chunk = blockIdx.x % nchunk;                                        \
    const long long b = blockIdx.x / nchunk;                                      \
    const int p = chunk * CC_THREADS + (int)threadIdx.x;                          \
    const bool active = p < HW;                                                   \
    const long long g = b * HW + p;

__global__ __launch_bounds__(CC_THREADS) void cc_init_kernel(Planes pl, int HW, int nchunk) {
    CC_PIXEL
    if (!active) return;
    pl.parent[g] = p;
    pl.size[g] = 0;
    pl.visited[g] = -1;
    if (p == 0) pl.cursor[b] = 0;
}

__global__ __launch_bounds__(CC_THREADS) void cc_merge_kernel(const int64_t* __restrict__ labels, Planes pl, int HW, int W, int nchunk) {
    CC_PIXEL
    if (!active) return;
    const int64_t lab = labels[g];
    int* parent = pl.parent + b * HW;
    const int x = p % W;
    if (x + 1 < W && labels[g + 1] == lab) cc_unite(parent, p, p + 1);
    if (p + W < HW && labels[g + W] == lab) cc_unite(parent, p, p + W);
}

// the forest is final: parent <- root (a concurrent chase through this pixel reads the old parent or the root, both ancestors)
__global__ __launch_bounds__(CC_THREADS) void cc_flatten_kernel(Planes pl, int HW, int nchunk) {
    CC_PIXEL
    int r = -1;
    if (active) {
        r = cc_find(pl.parent + b * HW, p);
        pl.parent[g] = r;
    }
    // one add per run of equal roots among the wave's 64 consecutive pixels; lanes past the sample form a last run of -1
    const int lane = threadIdx.x & 63;
    const int before = __shfl_up(r, 1);
    const bool lead = lane == 0 || before != r;
    const u64_t leads = __ballot(lead);
    if (lead && r >= 0) {
        const u64_t later = lane == 63 ? 0ull : leads >> (lane + 1);
        atomicAdd(pl.size + b * HW + r, later ? __ffsll(later) : 64 - lane);
    }
}

__device__ __forceinline__ bool cc_kept_root(const Planes& pl, long long g, int p, bool active, int min_size) {
    return active && pl.parent[g] == p && pl.size[g] >= min_size;
}

__global__ __launch_bounds__(CC_THREADS) void cc_count_kernel(Planes pl, int HW, int nchunk, int min_size) {
    CC_PIXEL
    const int n = __syncthreads_count(cc_kept_root(pl, g, p, active, min_size));
    if (threadIdx.x == 0) pl.chunks[blockIdx.x] = n;
}

// chunks[b][:] <- its exclusive prefix, n_labels[b] <- the total.  One workgroup per sample, tiles of CC_THREADS counts.
__global__ __launch_bounds__(CC_THREADS) void cc_scan_kernel(Planes pl, int nchunk, int* __restrict__ n_labels) {
    __shared__ int s[CC_THREADS];
    __shared__ int carry;
    int* c = pl.chunks + (long long)blockIdx.x * nchunk;
    const int tid = threadIdx.x;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < nchunk; base += CC_THREADS) {
        const int i = base + tid;
        const int v = i < nchunk ? c[i] : 0;
        s[tid] = v;
        __syncthreads();
        for (int d = 1; d < CC_THREADS; d <<= 1) {
            const int t = tid >= d ? s[tid - d] : 0;
            __syncthreads();
            s[tid] += t;
            __syncthreads();
        }
        const int start = carry;
        if (i < nchunk) c[i] = start + s[tid] - v;
        __syncthreads();
        if (tid == CC_THREADS - 1) carry = start + s[tid];
        __syncthreads();
    }
    if (tid == 0 && n_labels) n_labels[blockIdx.x] = carry;
}

__global__ __launch_bounds__(CC_THREADS) void cc_rank_kernel(Planes pl, int HW, int nchunk, int min_size) {
    __shared__ int waves[CC_THREADS / 64];
    CC_PIXEL
    const bool kept = cc_kept_root(pl, g, p, active, min_size);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const u64_t m = __ballot(kept);
    if (lane == 0) waves[wave] = __popcll(m);
    __syncthreads();
    if (!kept) return;
    int at = pl.chunks[blockIdx.x] + __popcll(m & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) at += waves[w];
    pl.fin[g] = at;
}

__global__ __launch_bounds__(CC_THREADS) void cc_donor_kernel(Planes pl, int HW, int W, int nchunk, int min_size) {
    CC_PIXEL
    if (!active || pl.parent[g] != p) return;
    const int size = pl.size[g];
    if (size >= min_size) return;
    const int* root = pl.parent + b * HW;
    int* visited = pl.visited + b * HW;
    const int at = atomicAdd(pl.cursor + b, size);              // the small components of a sample hold at most HW pixels together
    int donor = -1;
    if (size >= 1 && at >= 0 && at <= HW - size) {
        int* queue = pl.queue + b * HW + at;                     // [size]
        queue[0] = p;
        int n = 1;
        for (int v = 0; v < n; ++v) {                            // n <= size throughout
            const int c = queue[v];
            const int cx = c % W;
            const int nb[4] = {cx + 1 < W ? c + 1 : -1, cx > 0 ? c - 1 : -1, c + W < HW ? c + W : -1, c - W};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int m = nb[k];
                if (m < 0) continue;
                const int rm = root[m];
                if (rm == p) {
                    if (m != p && visited[m] != p && n < size) {
                        visited[m] = p;
                        queue[n++] = m;
                    }
                } else if (rm < p) {
                    donor = rm;
                }
            }
        }
    }
    pl.fin[g] = donor < 0 ? CC_NO_DONOR : -1 - donor;
}

// fin is final: kept roots hold their rank, small ones their donor's root.  The result goes to the size plane.
__global__ __launch_bounds__(CC_THREADS) void cc_resolve_kernel(Planes pl, int HW, int nchunk) {
    CC_PIXEL
    if (!active || pl.parent[g] != p) return;
    const int* fin = pl.fin + b * HW;
    int c = fin[p];
    for (int r = p; c < 0 && c != CC_NO_DONOR;) {
        const int d = -1 - c;
        if (d >= r) { c = CC_NO_DONOR; break; }                  // never: a donor's root is below its taker's
        r = d;
        c = fin[r];
    }
    pl.size[g] = c == CC_NO_DONOR ? 0 : c;
}

__global__ __launch_bounds__(CC_THREADS) void cc_write_kernel(Planes pl, int HW, int nchunk, int64_t* __restrict__ out) {
    CC_PIXEL
    if (!active) return;
    out[g] = (int64_t)pl.size[b * HW + pl.parent[g]];
}

int cc_chunks(int HW) { return (HW + CC_THREADS - 1) / CC_THREADS; }

size_t cc_bytes(int B, int H, int W) {
    const size_t HW = (size_t)H * W;
    return ((size_t)B * HW * CC_PLANES + (size_t)B * cc_chunks((int)HW) + (size_t)B) * sizeof(int);
}

bool cc_geometry_ok(int B, int H, int W) {
    return B >= 1 && H >= 1 && W >= 1 && (long long)H * W <= CC_MAX_PIXELS && (long long)B * cc_chunks(H * W) <= 0x7fffffffLL;
}

int cc_check(const int64_t* labels, int B, int H, int W, int min_size, const int64_t* out, const void* workspace, size_t workspace_bytes) {
    if (!labels || !out || !workspace || out == labels || min_size < 0 || !cc_geometry_ok(B, H, W) || ((uintptr_t)workspace & 3))
        return OESS_EINVAL;
    return workspace_bytes < cc_bytes(B, H, W) ? OESS_ENOMEM : OESS_OK;
}

// the launches; marks (nullable): CC_PHASES + 1 events recorded around the phases
int cc_run(const int64_t* labels, int B, int H, int W, int min_size, int64_t* out, int* n_labels, void* workspace, size_t workspace_bytes,
           hipStream_t st, hipEvent_t* marks) {
    const int bad = cc_check(labels, B, H, W, min_size, out, workspace, workspace_bytes);
    if (bad != OESS_OK) return bad;
    const int HW = H * W, nchunk = cc_chunks(HW);
    const size_t plane = (size_t)B * HW;
    Planes pl;
    pl.parent = (int*)workspace;
    pl.size = pl.parent + plane;
    pl.fin = pl.size + plane;
    pl.queue = pl.fin + plane;
    pl.visited = pl.queue + plane;
    pl.chunks = pl.visited + plane;
    pl.cursor = pl.chunks + (size_t)B * nchunk;
    const dim3 grid((unsigned)((long long)B * nchunk)), block(CC_THREADS);
    int phase = 0;
#define CC_MARK() do { if (marks) OESS_HIP(hipEventRecord(marks[phase++], st)); } while (0)
    CC_MARK();
    hipLaunchKernelGGL(cc_init_kernel, grid, block, 0, st, pl, HW, nchunk);
    hipLaunchKernelGGL(cc_merge_kernel, grid, block, 0, st, labels, pl, HW, W, nchunk);
    CC_MARK();
    hipLaunchKernelGGL(cc_flatten_kernel, grid, block, 0, st, pl, HW, nchunk);
    CC_MARK();
    hipLaunchKernelGGL(cc_count_kernel, grid, block, 0, st, pl, HW, nchunk, min_size);
    hipLaunchKernelGGL(cc_scan_kernel, dim3(B), block, 0, st, pl, nchunk, n_labels);
    hipLaunchKernelGGL(cc_rank_kernel, grid, block, 0, st, pl, HW, nchunk, min_size);
    CC_MARK();
    hipLaunchKernelGGL(cc_donor_kernel, grid, block, 0, st, pl, HW, W, nchunk, min_size);
    CC_MARK();
    hipLaunchKernelGGL(cc_resolve_kernel, grid, block, 0, st, pl, HW, nchunk);
    hipLaunchKernelGGL(cc_write_kernel, grid, block, 0, st, pl, HW, nchunk, out);
    CC_MARK();
#undef CC_MARK
    OESS_HIP(hipGetLastError());
    return OESS_OK;
}
}  // namespace

extern "C" {

size_t oess_slic_connectivity_workspace_bytes(int B, int H, int W) {
    return cc_geometry_ok(B, H, W) ? cc_bytes(B, H, W) : 0;
}

int oess_slic_connectivity_i64(const int64_t* labels, int B, int H, int W, int min_size, int64_t* out, int* n_labels, void* workspace,
                               size_t workspace_bytes, oess_stream_t stream) {
    return cc_run(labels, B, H, W, min_size, out, n_labels, workspace, workspace_bytes, (hipStream_t)stream, nullptr);
}

int oess_slic_connectivity_phase_ms(const int64_t* labels, int B, int H, int W, int min_size, int64_t* out, void* workspace,
                                    size_t workspace_bytes, float* phase_ms, oess_stream_t stream) {
    if (!phase_ms) return OESS_EINVAL;
    const int bad = cc_check(labels, B, H, W, min_size, out, workspace, workspace_bytes);
    if (bad != OESS_OK) return bad;                              // before any event is made
    hipEvent_t marks[CC_PHASES + 1] = {};
    int made = 0, rc = OESS_OK;
    for (; made <= CC_PHASES; ++made)
        if (hipEventCreate(&marks[made]) != hipSuccess) { rc = OESS_ELAUNCH; break; }
    if (rc == OESS_OK) rc = cc_run(labels, B, H, W, min_size, out, nullptr, workspace, workspace_bytes, (hipStream_t)stream, marks);
    if (rc == OESS_OK && hipEventSynchronize(marks[CC_PHASES]) != hipSuccess) rc = OESS_ELAUNCH;
    for (int i = 0; rc == OESS_OK && i < CC_PHASES; ++i)
        if (hipEventElapsedTime(&phase_ms[i], marks[i], marks[i + 1]) != hipSuccess) rc = OESS_ELAUNCH;
    for (int i = 0; i < made; ++i) (void)hipEventDestroy(marks[i]);
    return rc;
}

}  // extern "C"
