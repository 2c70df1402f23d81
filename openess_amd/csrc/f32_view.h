// fp32 inference files (conv_f32.hip, semseg_f32.hip, deeplab_f32.hip): the strided NHWC view their kernels take, the checks
// of the oess_f32_view_t arguments behind it, and V-channel vector access.  Included inside each file's anonymous namespace.

struct View {
    const float* p;
    long long sb, sy, sx, sc;
};

template <int V>
struct Vec {
    float v[V];
};

template <int V>
__device__ __forceinline__ Vec<V> ldv(const float* p) {
    Vec<V> r;
    if constexpr (V == 4) {
        const float4 t = *(const float4*)p;
        r.v[0] = t.x; r.v[1] = t.y; r.v[2] = t.z; r.v[3] = t.w;
    } else {
        r.v[0] = p[0];
    }
    return r;
}

template <int V>
__device__ __forceinline__ void stv(float* p, const Vec<V>& r) {
    if constexpr (V == 4) *(float4*)p = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
    else p[0] = r.v[0];
}

bool view_ok(const oess_f32_view_t* v) { return v && v->data; }

View to_view(const oess_f32_view_t* v) { return View{v->data, v->sb, v->sy, v->sx, v->sc}; }

// dense channels whose every pixel starts on a 16-byte boundary
bool vec_ok(const oess_f32_view_t* v) {
    return v->sc == 1 && ((uintptr_t)v->data & 15) == 0 && v->sb % 4 == 0 && v->sy % 4 == 0 && v->sx % 4 == 0;
}

bool geometry_ok(int B, int H, int W, int C) {
    return B >= 1 && B <= 65535 && H >= 1 && W >= 1 && C >= 1 && C <= (1 << 20) && (long long)H * W < (1LL << 30) &&
           (long long)B * H * W * C < (1LL << 40);
}
