// fp32 normalisation files (semseg_f32.hip, batchnorm_f32.hip): Chan's pairwise update of (count, mean, M2) and the fixed LDS
// tree that merges the threads of a workgroup which share channels.  Included inside each file's anonymous namespace, after
// its NT (threads per workgroup).

// Chan et al.: (na, ma, M2a) <- (na, ma, M2a) merged with (nb, mb, M2b)
template <int V>
__device__ __forceinline__ void chan(float& na, float (&ma)[V], float (&qa)[V], float nb, const float* mb, const float* qb) {
    if (nb == 0.f) return;
    if (na == 0.f) {
#pragma unroll
        for (int i = 0; i < V; ++i) { ma[i] = mb[i]; qa[i] = qb[i]; }
        na = nb;
        return;
    }
    const float n = na + nb, f = nb / n;
#pragma unroll
    for (int i = 0; i < V; ++i) {
        const float d = mb[i] - ma[i];
        ma[i] = ma[i] + d * f;
        qa[i] = qa[i] + qb[i] + d * d * (na * f);
    }
    na = n;
}

// merge the rows (threads with the same lane) of a workgroup; the result is in row 0.  sm: NT * (2 V + 1) floats
template <int V>
__device__ __forceinline__ void merge_rows(float& n, float (&m)[V], float (&q)[V], int tid, int lanes_log2, float* sm) {
    constexpr int S = 2 * V + 1;
    const int row = tid >> lanes_log2, rows = NT >> lanes_log2;
    float* me = sm + tid * S;
    me[0] = n;
#pragma unroll
    for (int i = 0; i < V; ++i) { me[1 + i] = m[i]; me[1 + V + i] = q[i]; }
    __syncthreads();
    for (int s = rows >> 1; s >= 1; s >>= 1) {
        if (row < s) {
            const float* o = sm + (tid + (s << lanes_log2)) * S;
            chan<V>(n, m, q, o[0], o + 1, o + 1 + V);
            me[0] = n;
#pragma unroll
            for (int i = 0; i < V; ++i) { me[1 + i] = m[i]; me[1 + V + i] = q[i]; }
        }
        __syncthreads();
    }
}
