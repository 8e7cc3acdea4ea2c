// Monotonic RNN-T loss (Tripathi et al. 2019) for gfx950: the forward-backward over the lattice the decoders here walk - every frame makes
// exactly ONE decision, blank or one label, and the emitting frame is consumed (include/ttmi.h has the recursion).  No reference
// counterpart: the reference trains the standard lattice alone (rnnt.hip), which this file leaves untouched.
//
//   mono_lse_kernel        HBM-bound: one wave per (b,t,u) row of V logits, lattice.h's row_lse walk (shared with rnnt_lse_kernel); emits lse
//                          and the row's two emission log-probs TIME-MAJOR ([b][t][u]): the recursion is frame-synchronous and reads one
//                          whole frame row per step (rnnt.hip's diagonal-major layout serves its anti-diagonal frontier, not this one).
//   mono_alphabeta_kernel  latency-bound dynamic programme: one wave per (utterance, direction), T_b serial steps (the standard lattice
//                          runs T_b + U_b - 1).  Lane l, slot r owns label u = 64 r + l; the frontier of one frame lives in registers, the
//                          u-1 / u+1 neighbour arrives by a one-lane DPP wave rotate, and the cell that crosses a slot seam is the rotate's
//                          wrapped lane of the neighbouring slot (a select, no LDS).  Emission rows are prefetched PF frames ahead.
//   mono_grad_kernel       HBM-bound: one wave per row reads the logits once and writes the gradient once (in place allowed).
//   mono_viterbi_kernel    forced alignment: the alpha walk with max in place of log-add-exp, one ballot word of decisions per frame and slot,
//                          and the backtrace, in one launch (one wave per utterance).
//   mono_emit_stats_kernel expected emission frame of every label from alpha / beta, lanes across the labels of a frame row.
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
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * MONO_WAVES + (threadIdx.x >> 6);
    if (row >= (long)B * T * U1) return;
    const LatticeRow p = lattice_row(row, T, U1, act_lens, label_lens);
    if (!p.inside()) return;               // (the lattice walk and the gradient never read these entries)
    const int b = p.b, u = p.u, Ub = p.Ub;
    const TL* r = logits + row * ldv;
    float M, s;
    row_lse<TL>(r, V, vec_ok, lane, M, s);
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

// ------------------------------------------------------------------ gradient
template <typename TL>
__global__ __launch_bounds__(MONO_WAVES * 64) void mono_grad_kernel(
    const TL* logits, long ldv, const int* __restrict__ labels, const int* __restrict__ act_lens, const int* __restrict__ label_lens,
    int B, int T, int U1, int V, int blank, int vec_ok, const float* __restrict__ lse, const acc_t* __restrict__ alpha_g,
    const acc_t* __restrict__ beta_g, const acc_t* __restrict__ ll, const float* __restrict__ grad_out, int grad_out_stride, float scale,
    TL* grad, long ldg) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * MONO_WAVES + (threadIdx.x >> 6);
    if (row >= (long)B * T * U1) return;
    const LatticeRow p = lattice_row(row, T, U1, act_lens, label_lens);
    const int b = p.b, t = p.t, u = p.u, Ub = p.Ub;
    const acc_t L = ll[b];
    // rows outside the lattice and utterances without a path (U_b > T_b): zero rows
    const bool valid = p.inside() && !(L <= MONO_DEAD);
    const TL* r = logits + row * ldv;
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
    row_map<TL>(r, grad + row * ldg, V, ldg, vec_ok, lane, valid, [&](float x, int v) -> float {
        float e = __expf(x + c);
        e -= (v == blank) ? eb : 0.f;
        e -= (v == yv) ? el : 0.f;
        return valid ? gs * e : 0.f;
    });
}

// ------------------------------------------------------------------ forced alignment: best path through the monotonic lattice
// v(0,0) = 0, v(t+1,u) = max(v(t,u) + lpb(t,u), v(t,u-1) + lpl(t,u-1)); the label move is taken only when it is STRICTLY greater (a tie goes
// to blank).  It is the alpha half of mono_alphabeta_kernel with max in place of lae, in the same shape: one wave per utterance, lane l / slot
// r owns label u = 64 r + l, the frontier in fp64 registers, the label term formed by its owner and rotated one lane, the slot seam a select
// between two rotated registers, emission rows prefetched PF frames ahead (unconditional loads of a clamped index; what they bring from
// outside the ragged lattice is dropped by selects, never by arithmetic).
// The decision of a cell is one bit (1 = cell (t+1, u) was reached by the label move of frame t); per frame and slot that is one __ballot word,
// stored by lane 0 at dec[t * W + r] - in LDS when the utterance's words fit, else in the caller's workspace.  The backtrace follows in the same
// kernel: every move steps one frame down, so the path crosses frames T_b - 1 ... 0 in order, one decision each; the wave fetches the words of
// 64 frames at a time (lane j: frame t - j, slot u / 64) and walks them by lane reads with t and u in scalar registers - a new fetch only after
// 64 steps or when u leaves the slot.  The walk keeps u <= t + 1: with u = t + 1 labels left the move is a label whatever the bit says, with
// u = 0 it is a blank, so it emits exactly U_b labels at strictly decreasing frames and ends at (0, 0) whatever the data (NaN included).
typedef unsigned long long dec_t;

template <int R, int PF, bool LDS_DEC>
__global__ __launch_bounds__(64) void mono_viterbi_kernel(const float* __restrict__ lpb_g, const float* __restrict__ lpl_g,
                                                          const int* __restrict__ act_lens, const int* __restrict__ label_lens, int T, int U1,
                                                          int W, dec_t* __restrict__ dec_ws, int* __restrict__ frames,
                                                          float* __restrict__ score, int backtrace) {
    extern __shared__ __attribute__((aligned(16))) char mono_vit_smem[];
    const int b = blockIdx.x;
    const int lane = threadIdx.x;
    const int Tb = clampi(act_lens[b], 1, T), Ub = clampi(label_lens[b], 0, U1 - 1);
    const float* lpb = lpb_g + (long)b * T * U1;
    const float* lpl = lpl_g + (long)b * T * U1;
    dec_t* dec_l = reinterpret_cast<dec_t*>(mono_vit_smem);                 // [T_b][W] (LDS_DEC)
    dec_t* dec_g = dec_ws + (long)b * T * W;                                // [T][W] per utterance (otherwise)
    int* fr = frames + (long)b * (U1 - 1);
    const bool no_path = Ub > Tb;                                           // wave-uniform: more labels than frames
    for (int u = (no_path ? 0 : Ub) + lane; u < U1 - 1; u += 64) fr[u] = -1;      // labels the utterance does not have
    if (no_path) {
        if (lane == 0) score[b] = -INFINITY;
        return;
    }
    bool vb[R], vl[R];                     // this slot's cell exists / has a label move
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int u = r * 64 + lane;
        vb[r] = u <= Ub;
        vl[r] = u < Ub;
    }
    MonoRows<R, PF> cur, nxt;
    acc_t a[R];
#pragma unroll
    for (int r = 0; r < R; ++r) a[r] = (r == 0 && lane == 0) ? 0.0 : (acc_t)NEG;
    mono_load_rows<R, PF>(cur, lpb, lpl, 0, 1, Tb, U1, lane);
    for (int base = 0; base < Tb; base += PF) {
        mono_load_rows<R, PF>(nxt, lpb, lpl, base + PF, 1, Tb, U1, lane);
#pragma unroll
        for (int s = 0; s < PF; ++s) {
            const int t = base + s;
            if (t < Tb) {                  // wave-uniform
                acc_t x[R];
#pragma unroll
                for (int r = 0; r < R; ++r) x[r] = rot_r1(vl[r] ? a[r] + (acc_t)cur.pl[s][r] : (acc_t)NEG);
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    // lane 0 of slot r: the wrapped lane 63 of slot r-1 (label 64 r - 1); nothing left of label 0
                    const acc_t left = (lane == 0) ? (r > 0 ? x[r > 0 ? r - 1 : 0] : (acc_t)NEG) : x[r];
                    const acc_t tt = a[r] + (acc_t)cur.pb[s][r];
                    const bool lab = vb[r] && (r > 0 || lane > 0) && (left > tt);      // strictly greater: a tie goes to blank
                    a[r] = vb[r] ? (lab ? left : tt) : (acc_t)NEG;
                    const dec_t w = __ballot(lab);
                    if (r < W && lane == 0) {
                        if constexpr (LDS_DEC) dec_l[t * W + r] = w;
                        else dec_g[(long)t * W + r] = w;
                    }
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
        if (r * 64 + lane == Ub) score[b] = a[r] <= MONO_DEAD ? -INFINITY : (float)a[r];      // no terminal blank (a NaN stays a NaN)
    if (!backtrace) return;          // measurement only (ttmi_set_option(23, 2)): the forward walk alone
    if constexpr (!LDS_DEC) __threadfence();
    __syncthreads();                 // lane 0's decision words are visible to the whole wave
    int t = Tb - 1, u = Ub;          // the move into (t + 1, u) is frame t's decision
    while (t >= 0) {
        const int g = u >> 6;
        const int tl = t - lane;
        dec_t w = 0;
        if (tl >= 0) {
            if constexpr (LDS_DEC) w = dec_l[tl * W + g];
            else w = dec_g[(long)tl * W + g];
        }
        const int wlo = (int)(unsigned)(w & 0xffffffffULL), whi = (int)(unsigned)(w >> 32);
        for (int j = 0; j < 64 && t >= 0 && (u >> 6) == g; ++j, --t) {
            const unsigned lo = (unsigned)__builtin_amdgcn_readlane(wlo, j), hi = (unsigned)__builtin_amdgcn_readlane(whi, j);
            const unsigned bit = (((u & 32) ? hi : lo) >> (u & 31)) & 1u;
            if (u > 0 && (bit || u > t)) {      // (t, u - 1) -> (t + 1, u): label u is frame t's decision (forced once u = t + 1 labels are left)
                if (lane == 0) fr[u - 1] = t;
                --u;
            }
        }
    }
}

// Per label, the posterior over its emission frame from a finished forward: e(t,u) = exp(alpha(t,u) + lpl(t,u) + beta(t+1,u+1) - ll), u < U_b.
// mass = sum_t e (every path emits every label exactly once: 1, a health check of the lattice), expected = sum_t t e.  One workgroup per
// (utterance, 64 labels): lanes across u, so every load of the time-major tables is one coalesced row segment; wave w takes frames w,
// w + MONO_ES_WAVES, ... in order, and the partial sums meet in LDS, added by wave 0 in wave order - fp64 throughout, the same order in
// every run, no atomics.  Entries u >= U_b and utterances without a path: mass 0, expected -1.
constexpr int MONO_ES_WAVES = 16;

__global__ __launch_bounds__(MONO_ES_WAVES * 64) void mono_emit_stats_kernel(
    const acc_t* __restrict__ alpha_g, const acc_t* __restrict__ beta_g, const acc_t* __restrict__ ll, const float* __restrict__ lpl_g,
    const int* __restrict__ act_lens, const int* __restrict__ label_lens, int T, int U1, int G, float* __restrict__ expected,
    float* __restrict__ mass) {
    __shared__ acc_t part[2][MONO_ES_WAVES][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int b = blockIdx.x / G;
    const int u = (blockIdx.x % G) * 64 + lane;
    const int Tb = clampi(act_lens[b], 1, T), Ub = clampi(label_lens[b], 0, U1 - 1);
    const acc_t L = ll[b];
    const bool live = !(Ub > Tb) && !(L <= MONO_DEAD);      // wave-uniform
    acc_t m = 0.0, e1 = 0.0;
    if (live && u < Ub) {
        const acc_t* al = alpha_g + (long)b * (T + 1) * U1 + u;
        const acc_t* be = beta_g + (long)b * (T + 1) * U1 + U1 + u + 1;      // beta(t + 1, u + 1)
        const float* pl = lpl_g + (long)b * T * U1 + u;
#pragma unroll 4
        for (int t = wv; t < Tb; t += MONO_ES_WAVES) {
            const long o = (long)t * U1;
            const acc_t e = (acc_t)__expf((float)(al[o] + (acc_t)pl[o] + be[o] - L));
            m += e;
            e1 += (acc_t)t * e;
        }
    }
    part[0][wv][lane] = m;
    part[1][wv][lane] = e1;
    __syncthreads();
    if (wv == 0 && u < U1 - 1) {
        m = part[0][0][lane];
        e1 = part[1][0][lane];
#pragma unroll
        for (int k = 1; k < MONO_ES_WAVES; ++k) {
            m += part[0][k][lane];
            e1 += part[1][k][lane];
        }
        const bool has = live && u < Ub;
        mass[(long)b * (U1 - 1) + u] = has ? (float)m : 0.f;
        expected[(long)b * (U1 - 1) + u] = has ? (float)e1 : -1.f;
    }
}

__host__ __device__ __forceinline__ size_t mono_dec_bytes(int T, int U1) { return (size_t)T * ((U1 + 63) / 64) * sizeof(dec_t); }

}  // namespace

int ttmi_rnnt_get_align_debug();          // rnnt.hip: ttmi_set_option(23, bits), shared with ttmi_rnnt_align

extern "C" {

// Forced alignment and emission statistics from the workspace a finished ttmi_mono_loss_fwd left on the same (B, T, U1); that workspace is
// only read (include/ttmi.h).  No host synchronisation, no memset node: both are capturable in a HIP graph.
size_t ttmi_mono_align_workspace_bytes(int B, int T, int U1) {
    if (B <= 0 || T <= 0 || U1 <= 0) return 0;
    return (size_t)B * mono_dec_bytes(T, U1);
}

int ttmi_mono_align(const void* workspace, const int* act_lens, const int* label_lens, int B, int T, int U1, void* align_workspace,
                    int* frames, float* score, void* stream) {
    TTMI_REQUIRE(workspace && act_lens && label_lens && align_workspace && (frames || U1 == 1) && score, "mono_align: null pointer");
    TTMI_REQUIRE(B > 0 && T > 0 && U1 > 0, "mono_align: bad shape B=%d T=%d U1=%d", B, T, U1);
    TTMI_REQUIRE(U1 <= 1024, "mono_align: U+1=%d > 1024 unsupported", U1);
    TTMI_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0 && (reinterpret_cast<uintptr_t>(align_workspace) & 7) == 0,
                 "mono_align: workspaces must be 8-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const MonoWs w = mono_carve(const_cast<void*>(workspace), B, T, U1);
    dec_t* dec = static_cast<dec_t*>(align_workspace);
    const int rc = with_slots(U1, [&](auto R, auto PF) {
        return launch_dec_lds("mono align", mono_viterbi_kernel<R, PF, true>, mono_viterbi_kernel<R, PF, false>, mono_dec_bytes(T, U1),
                              ttmi_rnnt_get_align_debug(), dim3(B), dim3(64), st, w.lpb, w.lpl, act_lens, label_lens, T, U1, (U1 + 63) / 64,
                              dec, frames, score);
    });
    if (rc) return rc;
    TTMI_LAUNCH_CHECK("mono_viterbi_kernel");
    return TTMI_OK;
}

int ttmi_mono_emit_stats(const void* workspace, const int* act_lens, const int* label_lens, int B, int T, int U1, float* expected,
                         float* mass, void* stream) {
    TTMI_REQUIRE(workspace && act_lens && label_lens && ((expected && mass) || U1 == 1), "mono_emit_stats: null pointer");
    TTMI_REQUIRE(B > 0 && T > 0 && U1 > 0, "mono_emit_stats: bad shape B=%d T=%d U1=%d", B, T, U1);
    TTMI_REQUIRE(U1 <= 1024, "mono_emit_stats: U+1=%d > 1024 unsupported", U1);
    TTMI_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "mono_emit_stats: workspace must be 8-byte aligned");
    if (U1 == 1) return TTMI_OK;          // no labels: nothing to write
    const MonoWs w = mono_carve(const_cast<void*>(workspace), B, T, U1);
    const int G = (U1 - 1 + 63) / 64;
    hipLaunchKernelGGL(mono_emit_stats_kernel, dim3((unsigned)((long)B * G)), dim3(MONO_ES_WAVES * 64), 0, static_cast<hipStream_t>(stream), w.alpha,
                       w.beta, w.ll, w.lpl, act_lens, label_lens, T, U1, G, expected, mass);
    TTMI_LAUNCH_CHECK("mono_emit_stats_kernel");
    return TTMI_OK;
}

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
    const int vec_ok = rows_vec_ok(logits, dtype == 0 ? 4 : 2);
    by_dtype(dtype, [&](auto z) {
        using TL = decltype(z);
        hipLaunchKernelGGL(mono_lse_kernel<TL>, dim3(cdiv(rows, MONO_WAVES)), dim3(MONO_WAVES * 64), 0, st, static_cast<const TL*>(logits), ldv,
                           labels, act_lens, label_lens, B, T, U1, V, blank, vec_ok, w.lse, w.lpb, w.lpl);
    });
    TTMI_LAUNCH_CHECK("mono_lse_kernel");
    with_slots(U1, [&](auto R, auto PF) {
        hipLaunchKernelGGL((mono_alphabeta_kernel<R, PF>), dim3(2 * B), dim3(64), 0, st, w.lpb, w.lpl, act_lens, label_lens, T, U1, w.alpha,
                           w.beta, w.ll, costs);
    });
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
    const int vec_ok = rows_vec_ok(logits, grad, ldv, ldg, dtype == 0 ? 4 : 2);
    by_dtype(dtype, [&](auto z) {
        using TL = decltype(z);
        hipLaunchKernelGGL(mono_grad_kernel<TL>, dim3(cdiv(rows, MONO_WAVES)), dim3(MONO_WAVES * 64), 0, st, static_cast<const TL*>(logits), ldv,
                           labels, act_lens, label_lens, B, T, U1, V, blank, vec_ok, w.lse, w.alpha, w.beta, w.ll, grad_out, grad_out_stride,
                           scale, static_cast<TL*>(grad), ldg);
    });
    TTMI_LAUNCH_CHECK("mono_grad_kernel");
    return TTMI_OK;
}

}  // extern "C"
