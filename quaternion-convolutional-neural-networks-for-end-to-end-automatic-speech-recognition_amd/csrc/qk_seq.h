// What the sequence kernels (qk_qlstm.hip, qk_qlnorm.hip, qk_qattn.hip, qk_qdwconv.hip, qk_rnnt.hip) share: 16-byte register groups,
// the 16x16x32 MFMA of both 16-bit types, and the host-side checks of their entry points.  Only helpers that are the SAME code in
// every file live here; what differs in arithmetic or evaluation order stays in its file ("The sequence kernels' shared
// header").  The CTC files (qk_ctc.hip, qk_ctc_align.hip, qk_ctc_decode.hip) and qk_api.hip use the host side only: the dtype
// dispatch and the argument checks.
#pragma once

#include "qk_common.h"

namespace qk {

// ---- device: 16-byte register groups ------------------------------------------------------------------------------------------------
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x8 __attribute__((ext_vector_type(8)));

template <typename T>
__device__ __forceinline__ uint4 load16(const T *p) { return *reinterpret_cast<const uint4 *>(p); }
template <typename T>
__device__ __forceinline__ void store16(T *p, const uint4 &v) { *reinterpret_cast<uint4 *>(p) = v; }

// V activation elements in one 16-byte register group
template <typename T> struct Vec16;
template <> struct Vec16<float> {
    static constexpr int V = 4;
    static __device__ __forceinline__ void unpack(const uint4 &r, float (&o)[4])
    {
        o[0] = __uint_as_float(r.x); o[1] = __uint_as_float(r.y); o[2] = __uint_as_float(r.z); o[3] = __uint_as_float(r.w);
    }
    static __device__ __forceinline__ uint4 pack(const float (&v)[4])
    {
        return make_uint4(__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3]));
    }
};
template <> struct Vec16<bf16> {
    static constexpr int V = 8;
    static __device__ __forceinline__ void unpack(const uint4 &r, float (&o)[8])
    {
        const unsigned w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) { o[2 * i] = __uint_as_float(w[i] << 16); o[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u); }
    }
    static __device__ __forceinline__ uint4 pack(const float (&v)[8])
    {
        // round-to-nearest-even by the packed conversion instruction of gfx950 (the integer form of from_f32<bf16> is ~6 VALU
        // operations per element).  The two differ on NaN payloads, so neither replaces the other where it is used.
        f32x8 f;
#pragma unroll
        for (int i = 0; i < 8; ++i) f[i] = v[i];
        return __builtin_bit_cast(uint4, __builtin_convertvector(f, bf16x8));
    }
};
template <> struct Vec16<f16> {
    static constexpr int V = 8;
    static __device__ __forceinline__ void unpack(const uint4 &r, float (&o)[8])
    {
        const f16x8 h = __builtin_bit_cast(f16x8, r);
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = (float)h[i];
    }
    static __device__ __forceinline__ uint4 pack(const float (&v)[8])
    {
        f16x8 h;
#pragma unroll
        for (int i = 0; i < 8; ++i) h[i] = (f16)v[i];
        return __builtin_bit_cast(uint4, h);
    }
};

// ---- device: matrix core ------------------------------------------------------------------------------------------------------------
// c += a . b on v_mfma_f32_16x16x32, operands as 16-byte fragments; the tag selects the 16-bit type
__device__ __forceinline__ floatx4 mfma16(bf16, const uint4 &a, const uint4 &b, const floatx4 &c)
{
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}
__device__ __forceinline__ floatx4 mfma16(f16, const uint4 &a, const uint4 &b, const floatx4 &c)
{
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
}
// the value a 16-bit path keeps at a rounding point (fp32: unchanged)
template <typename T> __device__ __forceinline__ float round_to(float v) { return to_f32(from_f32<T>(v)); }
template <> __device__ __forceinline__ float round_to<float>(float v) { return v; }

// ---- host: argument checks ----------------------------------------------------------------------------------------------------------
inline bool aligned(const void *p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
inline bool dtype_known(int dtype) { return dtype == QK_F32 || dtype == QK_BF16 || dtype == QK_F16; }
inline size_t elem_size(int dtype) { return dtype == QK_F32 ? 4 : 2; }
inline int vec_width(int dtype) { return dtype == QK_F32 ? 4 : 8; }          // Vec16<T>::V of the dtype
inline size_t align256(size_t n) { return (n + 255) / 256 * 256; }

// the head of every descriptor check (D: any of the qk_q*_desc_t, which all carry `dtype`)
template <typename D>
inline bool desc_head_ok(const D *d, const char *what)
{
    if (!d) { set_error("%s: NULL descriptor", what); return false; }
    if (!dtype_known(d->dtype)) { set_error("%s: unknown dtype %d", what, d->dtype); return false; }
    return true;
}

// the tail of every *_workspace_bytes
inline size_t bad_op(const char *what, int op)
{
    set_error("%s: op must be QK_OP_FWD or QK_OP_BWD (got %d)", what, op);
    return 0;
}

inline int workspace_ok(const char *what, const void *ws, size_t given, size_t need)
{
    if (ws && given >= need) return QK_OK;
    set_error("%s: workspace of %zu bytes needed, %zu given", what, need, given);
    return QK_ERR_WORKSPACE;
}

// the status of everything an entry point has launched
inline int launched(const char *what)
{
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return QK_OK;
    set_error("%s: kernel launch failed: %s", what, hipGetErrorString(e));
    return QK_ERR_LAUNCH;
}

// ---- host: dtype dispatch -----------------------------------------------------------------------------------------------------------
// f(T{}) with T the element type of a KNOWN dtype: `by_dtype(dtype, [&](auto t) { launch<decltype(t)>(...); })`
template <typename F>
inline void by_dtype(int dtype, F &&f)
{
    if (dtype == QK_F32) f(float{});
    else if (dtype == QK_BF16) f(bf16{});
    else f(f16{});
}
// the matrix-core paths: a 16-bit dtype
template <typename F>
inline void by_dtype16(int dtype, F &&f)
{
    if (dtype == QK_BF16) f(bf16{});
    else f(f16{});
}

}  // namespace qk
