// Pieces shared by the lattice losses (rnnt.hip, ctc.hip): the fp64 frontier and its log-add-exp, the one-lane DPP wave rotates, and the
// 16-byte row walk over f32 / bf16 logits rows of any alignment.
#pragma once
#include "common.h"

namespace ttmi_lattice {

constexpr float NEG = -1e30f;

// The frontier is carried in fp64: |alpha| grows to hundreds/thousands, where an fp32 ulp
// (6e-5 at 600) accumulated over T+U steps costs 1e-4 relative in exp(alpha+beta-ll).  Only the
// bounded correction log(1+exp(-|a-b|)) in [0, ln 2] is evaluated in fp32 (v_exp_f32/v_log_f32).
typedef double acc_t;
__device__ __forceinline__ acc_t lae(acc_t a, acc_t b) {
    const acc_t m = a > b ? a : b;
    const float d = -(float)fabs(a - b);
    return m + (acc_t)__logf(1.0f + __expf(d));
}

template <int CTRL>
__device__ __forceinline__ acc_t dpp_rot(acc_t x) {
    const long long v = __double_as_longlong(x);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(v & 0xffffffffLL), CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(v >> 32), CTRL, 0xF, 0xF, false);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
__device__ __forceinline__ acc_t rot_r1(acc_t x) { return dpp_rot<0x13C>(x); }   // lane l <- l-1 (0 <- 63): wave_ror:1
__device__ __forceinline__ acc_t rot_l1(acc_t x) { return dpp_rot<0x134>(x); }   // lane l <- l+1 (63 <- 0): wave_rol:1

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ------------------------------------------------------------------ row access helpers (f32 or bf16 logits)
typedef unsigned u32x4n __attribute__((ext_vector_type(4)));
template <typename TL>
struct Vec16 {                                   // one 16-byte access = NV elements
    static constexpr int NV = 16 / sizeof(TL);
    float f[NV];
    template <bool NT = true>
    __device__ __forceinline__ void load(const TL* p) {
        // the logits / gradient stream through once per pass (7 - 56 GB): streaming accesses in the gradient pass (its loads and stores
        // together: 4.19 -> 4.06 ms for the loss op); the log-sum-exp pass reads faster with plain loads (1.38 against 1.53 ms)
        uint4 w;
        if constexpr (NT) {
            const u32x4n wn = __builtin_nontemporal_load(reinterpret_cast<const u32x4n*>(p));
            w = make_uint4(wn.x, wn.y, wn.z, wn.w);
        } else {
            w = *reinterpret_cast<const uint4*>(p);
        }
        if constexpr (sizeof(TL) == 4) {
            f[0] = __uint_as_float(w.x); f[1] = __uint_as_float(w.y); f[2] = __uint_as_float(w.z); f[3] = __uint_as_float(w.w);
        } else {
            const uint32_t u[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                f[2 * i] = __uint_as_float(u[i] << 16);
                f[2 * i + 1] = __uint_as_float(u[i] & 0xffff0000u);
            }
        }
    }
    __device__ __forceinline__ void store(TL* p) const {
        uint4 w;
        if constexpr (sizeof(TL) == 4) {
            w.x = __float_as_uint(f[0]); w.y = __float_as_uint(f[1]); w.z = __float_as_uint(f[2]); w.w = __float_as_uint(f[3]);
        } else {
            w.x = pack_bf16x2(f[0], f[1]); w.y = pack_bf16x2(f[2], f[3]);
            w.z = pack_bf16x2(f[4], f[5]); w.w = pack_bf16x2(f[6], f[7]);
        }
        __builtin_nontemporal_store(u32x4n{w.x, w.y, w.z, w.w}, reinterpret_cast<u32x4n*>(p));
    }
};
template <typename TL>
__device__ __forceinline__ float ldf(const TL* p) {
    if constexpr (sizeof(TL) == 4) return *p;
    else return bf16_to_f32(*p);
}
template <typename TL>
__device__ __forceinline__ void stf(TL* p, float v) {
    if constexpr (sizeof(TL) == 4) *p = v;
    else *p = f32_to_bf16(v);
}
// elements before the first 16-byte boundary of row pointer r (all V when vectors are not allowed)
template <typename TL>
__device__ __forceinline__ int row_head(const TL* r, int V, int vec_ok) {
    constexpr int NV = 16 / sizeof(TL);
    int head = vec_ok ? (int)((NV - ((reinterpret_cast<uintptr_t>(r) / sizeof(TL)) % NV)) % NV) : V;
    return head > V ? V : head;
}

}  // namespace ttmi_lattice
