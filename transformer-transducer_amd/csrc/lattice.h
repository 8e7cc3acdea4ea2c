// Pieces shared by the lattice losses (rnnt.hip, mono.hip, ctc.hip, distill.hip):
//   * the fp64 frontier and its log-add-exp, the one-lane DPP wave rotates;
//   * the 16-byte access to f32 / bf16 logits rows of any alignment (Vec16, ldf / stf, row_head) and the two walks of one row by one wave
//     built on it: row_lse (online log-sum-exp) and row_map (gradient: g[v] = f(r[v], v), pad columns zeroed).  The kernels keep their own
//     row terms, their lambdas and their lane-0 epilogues; what differs between the losses on purpose stays in them;
//   * lattice_row: row -> (b, t, u) and the utterance's clamped lengths;
//   * host side: rows_vec_ok (when the walks may use 16-byte accesses), by_dtype (one call site for the f32 / bf16 instantiations),
//     with_slots (the slots-per-lane / prefetch-depth ladder of the one-wave lattice walks) and launch_dec_lds (forced alignment: decision
//     words in LDS when they fit, else in the caller's workspace).
#pragma once
#include "common.h"
#include <type_traits>

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


// ------------------------------------------------------------------ one row, one wave: online log-sum-exp
// Scalar head up to the first 16-byte boundary, 16-byte vectors (one running-max update per vector), scalar tail, then the wave's max M and
// S = sum exp(x - M): the row's log-sum-exp is M + log S.  el(x, v) maps a head / tail element of column v, vec(x, v0) may edit the vector
// of columns v0 .. v0 + NV - 1 before it is summed.  Plain loads: see the timings in Vec16::load.
template <typename TL, typename El, typename Vec>
__device__ __forceinline__ void row_lse(const TL* __restrict__ r, int V, int vec_ok, int lane, float& M, float& S, El&& el, Vec&& vec) {
    constexpr int NV = Vec16<TL>::NV;
    float m = NEG, s = 0.f;
    auto upd = [&](float x) {
        const float mn = fmaxf(m, x);
        s = s * __expf(m - mn) + __expf(x - mn);
        m = mn;
    };
    const int head = row_head<TL>(r, V, vec_ok);
    for (int i = lane; i < head; i += 64) upd(el(ldf<TL>(r + i), i));
    const int nvec = (V - head) / NV;
    for (int i = lane; i < nvec; i += 64) {
        Vec16<TL> x;
        const int v0 = head + i * NV;
        x.template load<false>(r + v0);
        vec(x, v0);
        float mx = x.f[0];
#pragma unroll
        for (int k = 1; k < NV; ++k) mx = fmaxf(mx, x.f[k]);
        const float mn = fmaxf(m, mx);
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < NV; ++k) acc += __expf(x.f[k] - mn);
        s = s * __expf(m - mn) + acc;
        m = mn;
    }
    for (int i = head + nvec * NV + lane; i < V; i += 64) upd(el(ldf<TL>(r + i), i));
    M = wave_max(m);
    S = wave_sum(s * __expf(m - M));
}
template <typename TL>
__device__ __forceinline__ void row_lse(const TL* __restrict__ r, int V, int vec_ok, int lane, float& M, float& S) {
    row_lse<TL>(r, V, vec_ok, lane, M, S, [](float x, int) { return x; }, [](Vec16<TL>&, int) {});
}

// ------------------------------------------------------------------ one row, one wave: gradient
// g[v] = f(valid ? r[v] : 0, v) for v < V and g[v] = 0 for the pad columns [V, ldg), which the dgrad GEMMs run over.  A row that is not
// valid is not read.  g may be r (in place): every lane overwrites only the elements it has read itself - a caller whose row terms read
// r[...] puts a wave barrier between those reads and this walk.  fvec(x, v0) maps a whole vector (columns v0 .. v0 + NV - 1) in place.
template <typename TL, typename F, typename FV>
__device__ __forceinline__ void row_map(const TL* r, TL* g, int V, long ldg, int vec_ok, int lane, bool valid, F&& f, FV&& fvec) {
    constexpr int NV = Vec16<TL>::NV;
    const int head = row_head<TL>(r, V, vec_ok);
    for (int i = lane; i < head; i += 64) stf<TL>(g + i, f(valid ? ldf<TL>(r + i) : 0.f, i));
    const int nvec = (V - head) / NV;
    for (int i = lane; i < nvec; i += 64) {
        Vec16<TL> x;
        const int v0 = head + i * NV;
        if (valid) x.load(r + v0);
#pragma unroll
        for (int k = 0; k < NV; ++k) x.f[k] = valid ? x.f[k] : 0.f;
        fvec(x, v0);
        x.store(g + v0);
    }
    for (int i = head + nvec * NV + lane; i < V; i += 64) stf<TL>(g + i, f(valid ? ldf<TL>(r + i) : 0.f, i));
    for (int i = V + lane; i < ldg; i += 64) stf<TL>(g + i, 0.f);
}
template <typename TL, typename F>
__device__ __forceinline__ void row_map(const TL* r, TL* g, int V, long ldg, int vec_ok, int lane, bool valid, F&& f) {
    row_map<TL>(r, g, V, ldg, vec_ok, lane, valid, f, [&](Vec16<TL>& x, int v0) {
#pragma unroll
        for (int k = 0; k < Vec16<TL>::NV; ++k) x.f[k] = f(x.f[k], v0 + k);
    });
}

// ------------------------------------------------------------------ row -> lattice node
struct LatticeRow {
    int b, t, u;      // row = (b * T + t) * U1 + u
    int Tb, Ub;       // the utterance's frames and labels, clamped into the padded lattice
    __device__ __forceinline__ bool inside() const { return t < Tb && u <= Ub; }
};
__device__ __forceinline__ LatticeRow lattice_row(long row, int T, int U1, const int* __restrict__ act_lens, const int* __restrict__ label_lens) {
    LatticeRow p;
    p.u = (int)(row % U1);
    const long bt = row / U1;
    p.t = (int)(bt % T);
    p.b = (int)(bt / T);
    p.Tb = clampi(act_lens[p.b], 1, T);
    p.Ub = clampi(label_lens[p.b], 0, U1 - 1);
    return p;
}

// ------------------------------------------------------------------ host side
// read-only walk: vectors whenever the elements themselves are aligned (row_head finds each row's first 16-byte boundary)
inline int rows_vec_ok(const void* logits, size_t es) { return (reinterpret_cast<uintptr_t>(logits) % es) == 0 ? 1 : 0; }
// gradient walk: logits and grad rows must also share their 16-byte phase
inline int rows_vec_ok(const void* logits, const void* grad, long ldv, long ldg, size_t es) {
    return ((reinterpret_cast<uintptr_t>(logits) % 16) == (reinterpret_cast<uintptr_t>(grad) % 16) && ((ldv - ldg) * (long)es) % 16 == 0 &&
            rows_vec_ok(logits, es)) ? 1 : 0;
}

// fn(TL{}) with TL = float (dtype 0) or bf16_t (dtype 1): `using TL = decltype(z)` names the row kernel's instantiation
template <typename Fn>
void by_dtype(int dtype, Fn&& fn) {
    if (dtype == 0) fn(float{});
    else fn(bf16_t{});
}

// the one-wave lattice walks: lane l, slot r owns label u = 64 r + l.  fn(R, PF) with R = slots per lane (64 R >= U1 <= 1024) and
// PF = emission rows per prefetch chunk (shrinks as R grows, to stay in registers), both std::integral_constant
template <typename Fn>
auto with_slots(int U1, Fn&& fn) {
    using std::integral_constant;
    if (U1 <= 64) return fn(integral_constant<int, 1>{}, integral_constant<int, 8>{});
    if (U1 <= 128) return fn(integral_constant<int, 2>{}, integral_constant<int, 8>{});
    if (U1 <= 256) return fn(integral_constant<int, 4>{}, integral_constant<int, 4>{});
    if (U1 <= 512) return fn(integral_constant<int, 8>{}, integral_constant<int, 2>{});
    return fn(integral_constant<int, 16>{}, integral_constant<int, 1>{});
}

// Forced alignment keeps one utterance's decision words in dynamic LDS (k_lds, `bytes` of it) up to VIT_LDS_MAX, else in the caller's
// workspace (k_ws).  debug = ttmi_set_option(23, bits): 1 = the workspace whatever the shape, 2 = no backtrace (measurements / tests);
// `backtrace` is the kernels' last argument.
constexpr size_t VIT_LDS_MAX = 128 * 1024;      // of the CU's 160 KB
template <typename... KArgs, typename... Args>
int launch_dec_lds(const char* what, void (*k_lds)(KArgs...), void (*k_ws)(KArgs...), size_t bytes, int debug, dim3 grid, dim3 block,
                   hipStream_t st, Args... args) {
    const int backtrace = (debug & 2) ? 0 : 1;
    if (bytes <= VIT_LDS_MAX && !(debug & 1)) {
        if (bytes > 64 * 1024) {
            // above the default limit the attribute is needed, and it belongs to the current DEVICE: it is set on every such call (a host-side
            // call, no stream work) instead of being remembered per process
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_lds), hipFuncAttributeMaxDynamicSharedMemorySize, (int)VIT_LDS_MAX);
            if (e != hipSuccess) {
                ttmi_set_error("%s: cannot reserve %zu bytes of LDS: %s", what, bytes, hipGetErrorString(e));
                return (int)e;
            }
        }
        hipLaunchKernelGGL(k_lds, grid, block, bytes, st, args..., backtrace);
    } else {
        hipLaunchKernelGGL(k_ws, grid, block, 0, st, args..., backtrace);
    }
    return TTMI_OK;
}

}  // namespace ttmi_lattice
