// Monotonic RNN-T loss (Tripathi et al. 2019) for gfx950: the forward-backward over the lattice the decoders here walk - every frame makes
// exactly ONE decision, blank or one label, and the emitting frame is consumed (include/ttmi.h has the recursion).  No reference
// counterpart: the reference trains the standard lattice alone (rnnt.hip), which this file leaves untouched.
//
//   mono_lse_kernel        HBM-bound: one wave per (b,t,u) row of V logits, the 16-byte online log-sum-exp walk of rnnt_lse_kernel; emits lse
//                          and the row's two emission log-probs TIME-MAJOR ([b][t][u]): the recursion is frame-synchronous and reads one
//                          whole frame row per step (rnnt.hip's diagonal-major layout serves its anti-diagonal frontier, not this one).
//   mono_alphabeta_kernel  latency-bound dynamic programme: one wave per (utterance, direction), T_b serial steps (the standard lattice
//                          runs T_b + U_b - 1).  Lane l, slot r owns label u = 64 r + l; the frontier of one frame lives in registers, the
//                          u-1 / u+1 neighbour arrives by a one-lane DPP wave rotate, and the cell that crosses a slot seam is the rotate's
//                          wrapped lane of the neighbouring slot (a select, no LDS).  Emission rows are prefetched PF frames ahead.
//   mono_grad_kernel       HBM-bound: one wave per row reads the logits once and writes the gradient once (in place allowed).
#include "common.h"
#include "lattice.h"

namespace {

using namespace ttmi_lattice;

constexpr int MONO_WAVES = 4;
constexpr acc_t MONO_DEAD = -1e29;        // a log-likelihood below this never met a live path (dead cells sit at or below NEG = -1e30)

struct MonoWs {
    acc_t *alpha, *beta, *ll;             // [B, T + 1, U1] x 2 (frame-major: row t holds alpha(t, 0 .. U1-1)), [B]
    float *lse, *lpb, *lpl;               // [B, T, U1] x 3
};
MonoWs mono_carve(void* ws, int B, int T, int U1) {
    const long n = (long)B * T * U1, na = (long)B * (T + 1) * U1;
    MonoWs w;
    acc_t* q = static_cast<acc_t*>(ws);   // fp64 part first (workspace must be 8-byte aligned)
    w.alpha = q; q += na;
    w.beta = q; q += na;
    w.ll = q; q += B;
    float* p = reinterpret_cast<float*>(q);
    w.lse = p; p += n;
    w.lpb = p; p += n;
    w.lpl = p;
    return w;
}

// ------------------------------------------------------------------ lse + gather
template <typename TL>
__global__ __launch_bounds__(MONO_WAVES * 64) void mono_lse_kernel(
    const TL* __restrict__ logits, long ldv, const int* __restrict__ labels, const int* __restrict__ act_lens,
    const int* __restrict__ label_lens, int B, int T, int U1, int V, int blank, int vec_ok, float* __restrict__ lse,
    float* __restrict__ lpb, float* __restrict__ lpl) {
    constexpr int NV = 16 / sizeof(TL);
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * MONO_WAVES + (threadIdx.x >> 6);
    if (row >= (long)B * T * U1) return;
    const int u = (int)(row % U1);
    const long bt = row / U1;
    const int t = (int)(bt % T);
    const int b = (int)(bt / T);
    const int Tb = clampi(act_lens[b], 1, T), Ub = clampi(label_lens[b], 0, U1 - 1);
    if (t >= Tb || u > Ub) return;         // (the lattice walk and the gradient never read these entries)
    const TL* r = logits + row * ldv;
    float m = NEG, s = 0.f;
    auto upd = [&](float x) {
        const float mn = fmaxf(m, x);
        s = s * __expf(m - mn) + __expf(x - mn);
        m = mn;
    };
    const int head = row_head<TL>(r, V, vec_ok);
    for (int i = lane; i < head; i += 64) upd(ldf<TL>(r + i));
    const int nvec = (V - head) / NV;
    for (int i = lane; i < nvec; i += 64) {
        Vec16<TL> x;
        x.template load<false>(r + head + i * NV);
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
    for (int i = head + nvec * NV + lane; i < V; i += 64) upd(ldf<TL>(r + i));
    const float M = wave_max(m);
    s = wave_sum(s * __expf(m - M));
    if (lane == 0) {
        const float l = M + __logf(s);
        lse[row] = l;
        // clamped at NEG so that a -inf logit is a dead transition and not an inf - inf in the log-add-exp (a NaN stays a NaN)
        const float pb = ldf<TL>(r + blank) - l;
        lpb[row] = pb < NEG ? NEG : pb;
        float pl = NEG;
        if (u < Ub) {
            const int y = clampi(labels[(long)b * (U1 - 1) + u], 0, V - 1);
            pl = ldf<TL>(r + y) - l;
            pl = pl < NEG ? NEG : pl;
        }
        lpl[row] = pl;
    }
}

// ------------------------------------------------------------------ alpha / beta
// R = slots per lane (64 R >= U1), PF = emission frames per prefetch chunk (shrinks as R grows, to stay in registers)
template <int R, int PF>
struct MonoRows {
    float pb[PF][R];
    float pl[PF][R];
};

// frames f0, f0 + dir, ... (clamped to [0, Tb - 1]: the loads past the utterance's end are unconditional and never used)
template <int R, int PF>
__device__ __forceinline__ void mono_load_rows(MonoRows<R, PF>& buf, const float* __restrict__ lpb, const float* __restrict__ lpl, int f0,
                                               int dir, int Tb, int U1, int lane) {
#pragma unroll
    for (int s = 0; s < PF; ++s) {
        const int t = clampi(f0 + dir * s, 0, Tb - 1);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int uc = min(r * 64 + lane, U1 - 1);         // in-range column for the lanes that pad the last slot
            buf.pb[s][r] = lpb[(long)t * U1 + uc];
            buf.pl[s][r] = lpl[(long)t * U1 + uc];
        }
    }
}

template <int R, int PF>
__global__ __launch_bounds__(64) void mono_alphabeta_kernel(const float* __restrict__ lpb_g, const float* __restrict__ lpl_g,
                                                            const int* __restrict__ act_lens, const int* __restrict__ label_lens, int T,
                                                            int U1, acc_t* __restrict__ alpha_g, acc_t* __restrict__ beta_g,
                                                            acc_t* __restrict__ ll, float* __restrict__ costs) {
    const int b = blockIdx.x >> 1;
    const bool do_beta = blockIdx.x & 1;
    const int lane = threadIdx.x;
    const int Tb = clampi(act_lens[b], 1, T), Ub = clampi(label_lens[b], 0, U1 - 1);
    const float* lpb = lpb_g + (long)b * T * U1;
    const float* lpl = lpl_g + (long)b * T * U1;
    acc_t* out = (do_beta ? beta_g : alpha_g) + (long)b * (T + 1) * U1;
    bool vb[R], vl[R], wr[R];              // this slot's cell exists / has a label move / is inside the stored row
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int u = r * 64 + lane;
        vb[r] = u <= Ub;
        vl[r] = u < Ub;
        wr[r] = u < U1;
    }
    MonoRows<R, PF> cur, nxt;
    acc_t a[R];
    if (!do_beta) {
        // alpha(t+1, u) = lae(alpha(t, u) + lpb(t, u), alpha(t, u-1) + lpl(t, u-1)): the label term is formed by its owner (u-1) and rotated
#pragma unroll
        for (int r = 0; r < R; ++r) {
            a[r] = (r == 0 && lane == 0) ? 0.0 : (acc_t)NEG;
            if (wr[r]) out[r * 64 + lane] = a[r];
        }
        mono_load_rows<R, PF>(cur, lpb, lpl, 0, 1, Tb, U1, lane);
        for (int base = 0; base < Tb; base += PF) {
            mono_load_rows<R, PF>(nxt, lpb, lpl, base + PF, 1, Tb, U1, lane);
#pragma unroll
            for (int s = 0; s < PF; ++s) {
                const int t = base + s;
                if (t < Tb) {              // wave-uniform
                    acc_t x[R];
#pragma unroll
                    for (int r = 0; r < R; ++r) x[r] = rot_r1(vl[r] ? a[r] + (acc_t)cur.pl[s][r] : (acc_t)NEG);
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        // lane 0 of slot r: the wrapped lane 63 of slot r-1 (label 64 r - 1); nothing left of label 0
                        const acc_t left = (lane == 0) ? (r > 0 ? x[r > 0 ? r - 1 : 0] : (acc_t)NEG) : x[r];
                        a[r] = vb[r] ? lae(a[r] + (acc_t)cur.pb[s][r], left) : (acc_t)NEG;
                        if (wr[r]) out[(long)(t + 1) * U1 + r * 64 + lane] = a[r];
                    }
                }
            }
#pragma unroll
            for (int s = 0; s < PF; ++s)
#pragma unroll
                for (int r = 0; r < R; ++r) { cur.pb[s][r] = nxt.pb[s][r]; cur.pl[s][r] = nxt.pl[s][r]; }
        }
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (r * 64 + lane == Ub) {
                ll[b] = a[r];
                costs[b] = a[r] <= MONO_DEAD ? INFINITY : (float)(-a[r]);      // U_b > T_b: no path, +inf (a NaN stays a NaN)
            }
    } else {
        // beta(t, u) = lae(lpb(t, u) + beta(t+1, u), lpl(t, u) + beta(t+1, u+1))
#pragma unroll
        for (int r = 0; r < R; ++r) {
            a[r] = (r * 64 + lane == Ub) ? 0.0 : (acc_t)NEG;
            if (wr[r]) out[(long)Tb * U1 + r * 64 + lane] = a[r];
        }
        mono_load_rows<R, PF>(cur, lpb, lpl, Tb - 1, -1, Tb, U1, lane);
        for (int base = Tb - 1; base >= 0; base -= PF) {
            mono_load_rows<R, PF>(nxt, lpb, lpl, base - PF, -1, Tb, U1, lane);
#pragma unroll
            for (int s = 0; s < PF; ++s) {
                const int t = base - s;
                if (t >= 0) {              // wave-uniform
                    acc_t x[R];
#pragma unroll
                    for (int r = 0; r < R; ++r) x[r] = rot_l1(a[r]);
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        // lane 63 of slot r: the wrapped lane 0 of slot r+1 (label 64 (r + 1)); nothing right of the last slot
                        const acc_t right = (lane == 63) ? (r + 1 < R ? x[r + 1 < R ? r + 1 : r] : (acc_t)NEG) : x[r];
                        const acc_t tl = vl[r] ? right + (acc_t)cur.pl[s][r] : (acc_t)NEG;
                        a[r] = vb[r] ? lae(a[r] + (acc_t)cur.pb[s][r], tl) : (acc_t)NEG;
                        if (wr[r]) out[(long)t * U1 + r * 64 + lane] = a[r];
                    }
                }
            }
#pragma unroll
            for (int s = 0; s < PF; ++s)
#pragma unroll
                for (int r = 0; r < R; ++r) { cur.pb[s][r] = nxt.pb[s][r]; cur.pl[s][r] = nxt.pl[s][r]; }
        }
    }
}

template <int R, int PF>
void mono_launch_alphabeta(hipStream_t st, int B, const MonoWs& w, const int* act_lens, const int* label_lens, int T, int U1,
                           float* costs) {
    hipLaunchKernelGGL((mono_alphabeta_kernel<R, PF>), dim3(2 * B), dim3(64), 0, st, w.lpb, w.lpl, act_lens, label_lens, T, U1, w.alpha,
                       w.beta, w.ll, costs);
}

// ------------------------------------------------------------------ gradient
template <typename TL>
__global__ __launch_bounds__(MONO_WAVES * 64) void mono_grad_kernel(
    const TL* logits, long ldv, const int* __restrict__ labels, const int* __restrict__ act_lens, const int* __restrict__ label_lens,
    int B, int T, int U1, int V, int blank, int vec_ok, const float* __restrict__ lse, const acc_t* __restrict__ alpha_g,
    const acc_t* __restrict__ beta_g, const acc_t* __restrict__ ll, const float* __restrict__ grad_out, int grad_out_stride, float scale,
    TL* grad, long ldg) {
    constexpr int NV = 16 / sizeof(TL);
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * MONO_WAVES + (threadIdx.x >> 6);
    if (row >= (long)B * T * U1) return;
    const int u = (int)(row % U1);
    const long bt = row / U1;
    const int t = (int)(bt % T);
    const int b = (int)(bt / T);
    const int Tb = clampi(act_lens[b], 1, T), Ub = clampi(label_lens[b], 0, U1 - 1);
    const acc_t L = ll[b];
    // rows outside the lattice and utterances without a path (U_b > T_b): zero rows
    const bool valid = (t < Tb) && (u <= Ub) && !(L <= MONO_DEAD);
    const TL* r = logits + row * ldv;
    TL* g = grad + row * ldg;
    float c = 0.f, eb = 0.f, el = 0.f, gs = 0.f;
    int yv = -1;
    if (valid) {
        const long ai = ((long)b * (T + 1) + t) * U1 + u;                       // (t, u); (t+1, u) is U1 further
        const float l = lse[row];
        const acc_t a = alpha_g[ai] - L;                                        // alpha - ll, fp64
        c = (float)(a + beta_g[ai]) - l;
        gs = scale * grad_out[(long)b * grad_out_stride];
        const float lpb = ldf<TL>(r + blank) - l;
        eb = __expf((float)(a + beta_g[ai + U1]) + lpb);                        // beta(t+1, u)
        if (u < Ub) {
            yv = clampi(labels[(long)b * (U1 - 1) + u], 0, V - 1);
            const float lpy = ldf<TL>(r + yv) - l;
            el = __expf((float)(a + beta_g[ai + U1 + 1]) + lpy);                // beta(t+1, u+1)
        }
    }
    // every lane has read r[blank], r[yv] before any lane overwrites them (in-place use)
    __builtin_amdgcn_wave_barrier();
    auto f = [&](float x, int v) -> float {
        float e = __expf(x + c);
        e -= (v == blank) ? eb : 0.f;
        e -= (v == yv) ? el : 0.f;
        return valid ? gs * e : 0.f;
    };
    const int head = row_head<TL>(r, V, vec_ok);
    for (int i = lane; i < head; i += 64) stf<TL>(g + i, f(valid ? ldf<TL>(r + i) : 0.f, i));
    const int nvec = (V - head) / NV;
    for (int i = lane; i < nvec; i += 64) {
        Vec16<TL> x;
        const int v0 = head + i * NV;
        if (valid) x.load(r + v0);
#pragma unroll
        for (int k = 0; k < NV; ++k) x.f[k] = f(valid ? x.f[k] : 0.f, v0 + k);
        x.store(g + v0);
    }
    for (int i = head + nvec * NV + lane; i < V; i += 64) stf<TL>(g + i, f(valid ? ldf<TL>(r + i) : 0.f, i));
    // padded pitch: columns [V, ldg) are zeroed so that the joint's dgrad GEMM may run over the full pitch
    for (int i = V + lane; i < ldg; i += 64) stf<TL>(g + i, 0.f);
}

}  // namespace

extern "C" {

// bytes of caller-provided workspace shared by ttmi_mono_loss_fwd / _bwd (8-byte aligned)
size_t ttmi_mono_workspace_bytes(int B, int T, int U1) {
    if (B <= 0 || T <= 0 || U1 <= 0) return 0;
    return sizeof(acc_t) * (2 * (size_t)B * (T + 1) * U1 + (size_t)B) + sizeof(float) * 3 * (size_t)B * T * U1 + 64;
}

int ttmi_mono_loss_fwd(const void* logits, int dtype, long ldv, const int* labels, const int* act_lens, const int* label_lens, int B, int T,
                       int U1, int V, int blank, void* workspace, float* costs, void* stream) {
    TTMI_REQUIRE(logits && (labels || U1 == 1) && act_lens && label_lens && workspace && costs, "mono_loss_fwd: null pointer");
    TTMI_REQUIRE(B > 0 && T > 0 && U1 > 0 && V > 0, "mono_loss_fwd: bad shape B=%d T=%d U1=%d V=%d", B, T, U1, V);
    TTMI_REQUIRE(ldv >= V && (dtype == 0 || dtype == 1), "mono_loss_fwd: bad pitch/dtype");
    TTMI_REQUIRE(blank >= 0 && blank < V, "mono_loss_fwd: blank %d outside [0,%d)", blank, V);
    TTMI_REQUIRE(U1 <= 1024, "mono_loss_fwd: U+1=%d > 1024 unsupported", U1);
    TTMI_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "mono_loss_fwd: workspace must be 8-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const MonoWs w = mono_carve(workspace, B, T, U1);
    const long rows = (long)B * T * U1;
    const size_t es = dtype == 0 ? 4 : 2;
    const int vec_ok = ((reinterpret_cast<uintptr_t>(logits) % es) == 0) ? 1 : 0;
    if (dtype == 0)
        hipLaunchKernelGGL(mono_lse_kernel<float>, dim3(cdiv(rows, MONO_WAVES)), dim3(MONO_WAVES * 64), 0, st,
                           static_cast<const float*>(logits), ldv, labels, act_lens, label_lens, B, T, U1, V, blank, vec_ok, w.lse, w.lpb,
                           w.lpl);
    else
        hipLaunchKernelGGL(mono_lse_kernel<bf16_t>, dim3(cdiv(rows, MONO_WAVES)), dim3(MONO_WAVES * 64), 0, st,
                           static_cast<const bf16_t*>(logits), ldv, labels, act_lens, label_lens, B, T, U1, V, blank, vec_ok, w.lse, w.lpb,
                           w.lpl);
    TTMI_LAUNCH_CHECK("mono_lse_kernel");
    if (U1 <= 64) mono_launch_alphabeta<1, 8>(st, B, w, act_lens, label_lens, T, U1, costs);
    else if (U1 <= 128) mono_launch_alphabeta<2, 8>(st, B, w, act_lens, label_lens, T, U1, costs);
    else if (U1 <= 256) mono_launch_alphabeta<4, 4>(st, B, w, act_lens, label_lens, T, U1, costs);
    else if (U1 <= 512) mono_launch_alphabeta<8, 2>(st, B, w, act_lens, label_lens, T, U1, costs);
    else mono_launch_alphabeta<16, 1>(st, B, w, act_lens, label_lens, T, U1, costs);
    TTMI_LAUNCH_CHECK("mono_alphabeta_kernel");
    return TTMI_OK;
}

int ttmi_mono_loss_bwd(const void* logits, int dtype, long ldv, const int* labels, const int* act_lens, const int* label_lens, int B, int T,
                       int U1, int V, int blank, const void* workspace, const float* grad_out, int grad_out_stride, float scale, void* grad,
                       long ldg, void* stream) {
    TTMI_REQUIRE(logits && (labels || U1 == 1) && act_lens && label_lens && workspace && grad_out && grad, "mono_loss_bwd: null pointer");
    TTMI_REQUIRE(B > 0 && T > 0 && U1 > 0 && V > 0, "mono_loss_bwd: bad shape B=%d T=%d U1=%d V=%d", B, T, U1, V);
    TTMI_REQUIRE(ldv >= V && ldg >= V && (dtype == 0 || dtype == 1), "mono_loss_bwd: bad pitch/dtype");
    TTMI_REQUIRE(blank >= 0 && blank < V, "mono_loss_bwd: blank %d outside [0,%d)", blank, V);
    TTMI_REQUIRE(U1 <= 1024, "mono_loss_bwd: U+1=%d > 1024 unsupported", U1);
    TTMI_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "mono_loss_bwd: workspace must be 8-byte aligned");
    TTMI_REQUIRE(logits != static_cast<const void*>(grad) || ldg == ldv, "mono_loss_bwd: in-place needs ldg == ldv");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const MonoWs w = mono_carve(const_cast<void*>(workspace), B, T, U1);
    const long rows = (long)B * T * U1;
    const size_t es = dtype == 0 ? 4 : 2;
    // vector path needs logits and grad rows to share their 16-byte phase
    const int vec_ok = ((reinterpret_cast<uintptr_t>(logits) % 16) == (reinterpret_cast<uintptr_t>(grad) % 16) &&
                        ((ldv - ldg) * (long)es) % 16 == 0 && (reinterpret_cast<uintptr_t>(logits) % es) == 0) ? 1 : 0;
    if (dtype == 0)
        hipLaunchKernelGGL(mono_grad_kernel<float>, dim3(cdiv(rows, MONO_WAVES)), dim3(MONO_WAVES * 64), 0, st,
                           static_cast<const float*>(logits), ldv, labels, act_lens, label_lens, B, T, U1, V, blank, vec_ok, w.lse, w.alpha,
                           w.beta, w.ll, grad_out, grad_out_stride, scale, static_cast<float*>(grad), ldg);
    else
        hipLaunchKernelGGL(mono_grad_kernel<bf16_t>, dim3(cdiv(rows, MONO_WAVES)), dim3(MONO_WAVES * 64), 0, st,
                           static_cast<const bf16_t*>(logits), ldv, labels, act_lens, label_lens, B, T, U1, V, blank, vec_ok, w.lse, w.alpha,
                           w.beta, w.ll, grad_out, grad_out_stride, scale, static_cast<bf16_t*>(grad), ldg);
    TTMI_LAUNCH_CHECK("mono_grad_kernel");
    return TTMI_OK;
}

}  // extern "C"
