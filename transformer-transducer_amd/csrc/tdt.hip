// Token-and-duration transducer (TDT; Xu et al., ICML 2023) for gfx950: the forward-backward over a lattice whose moves jump d frames, d from
// a fixed set of at most 8 durations in [1, 8], and the greedy decoder's frame-skipping pair (include/ttmi.h has the recursion and the
// decoder's rule).  A row of logits is V token columns followed by D duration columns, each sub-row normalised by itself.  With
// durations = (1) the lattice is mono.hip's.  No reference counterpart.
//
//   tdt_lse_kernel        HBM-bound: one wave per (b,t,u) row, lattice.h's row_lse walk on the V token columns and a register reduction on the D
//                         duration columns; emits lse_tok, lse_dur, lpb, lpl and ld_0 .. ld_{D-1} TIME-MAJOR ([b][t][u], one plane per table).
//   tdt_alphabeta_kernel  latency-bound dynamic programme: one wave per (utterance, direction), T_b serial steps.  Lane l, slot r owns label
//                         u = 64 r + l; the u-1 / u+1 neighbour arrives by a one-lane DPP wave rotate with the slot-seam select of mono.hip.
//                         A cell needs the frontier of up to 8 other frames: a ring of 8 frontier rows lives in LDS, and every lane reads and
//                         writes ITS OWN columns of it only (the neighbours come by the rotate), so the ring needs no barrier.  alpha PUSHES:
//                         frame s, once complete, adds its D outgoing moves into the pending rows s + d_j (contributions reach a row in the
//                         order of their source frames: one fixed summation order).  beta PULLS from the rows t + d_j.  Rows of alpha / beta
//                         are stored to the workspace for the gradient and never read back here.
//   tdt_grad_kernel       HBM-bound: one wave per row reads the row once and writes the gradient once (in place allowed).
//   tdt_scan_kernel       greedy decode: one wave per row of a block [B, n, V + D]: argmax and log-probability of both sub-rows.
//   tdt_advance_kernel    greedy decode: one thread per utterance follows the jumps through the block.
#include "common.h"
#include "lattice.h"
#include "rowops.h"

namespace {

using namespace ttmi_lattice;

constexpr int TDT_WAVES = 4;
constexpr int TDT_MAXD = 8;               // durations are in [1, TDT_MAXD], at most TDT_MAXD of them: the ring holds TDT_MAXD frontier rows
constexpr acc_t TDT_DEAD = -1e29;         // a log-likelihood below this never met a live path (dead cells sit at or below NEG = -1e30)

struct TdtDur {                           // copied into the launch: d[j] = duration j for j < n, 0 behind them
    int d[TDT_MAXD];
    int n;
};

struct TdtWs {
    acc_t *alpha, *beta, *ll;             // [B, T + 1, U1] x 2 (frame-major), [B]
    float *lse_tok, *lse_dur, *lpb, *lpl; // [B, T, U1] x 4
    float* ld;                            // [D][B, T, U1]: plane j holds log P(duration j)
};
TdtWs tdt_carve(void* ws, int B, int T, int U1) {
    const long n = (long)B * T * U1, na = (long)B * (T + 1) * U1;
    TdtWs w;
    acc_t* q = static_cast<acc_t*>(ws);   // fp64 part first (workspace must be 8-byte aligned)
    w.alpha = q; q += na;
    w.beta = q; q += na;
    w.ll = q; q += B;
    float* p = reinterpret_cast<float*>(q);
    w.lse_tok = p; p += n;
    w.lse_dur = p; p += n;
    w.lpb = p; p += n;
    w.lpl = p; p += n;
    w.ld = p;
    return w;
}

// the D duration logits of a row, by every lane (broadcast loads) -> their log-sum-exp; x[j] for j >= D is left at -inf
template <typename TL>
__device__ __forceinline__ float tdt_dur_lse(const TL* __restrict__ rd, int D, float (&x)[TDT_MAXD]) {
    float m = -INFINITY;
#pragma unroll
    for (int j = 0; j < TDT_MAXD; ++j) {
        x[j] = ldf<TL>(rd + (j < D ? j : D - 1));                // unconditional load at a clamped index, dropped by the select
        x[j] = j < D ? x[j] : -INFINITY;
        m = fmaxf(m, x[j]);
    }
    m = fmaxf(m, NEG);                                           // (an all -inf sub-row: exp(-inf - NEG) = 0, lse = -inf, every ld clamps at NEG)
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < TDT_MAXD; ++j) s += __expf(x[j] - m);
    return m + __logf(s);
}

// ------------------------------------------------------------------ lse + gather
template <typename TL>
__global__ __launch_bounds__(TDT_WAVES * 64) void tdt_lse_kernel(
    const TL* __restrict__ logits, long ldv, const int* __restrict__ labels, const int* __restrict__ act_lens,
    const int* __restrict__ label_lens, int B, int T, int U1, int V, int D, int blank, int vec_ok, float* __restrict__ lse_tok,
    float* __restrict__ lse_dur, float* __restrict__ lpb, float* __restrict__ lpl, float* __restrict__ ld) {
    const int lane = threadIdx.x & 63;
    const long rows = (long)B * T * U1;
    const long row = (long)blockIdx.x * TDT_WAVES + (threadIdx.x >> 6);
    if (row >= rows) return;
    const LatticeRow p = lattice_row(row, T, U1, act_lens, label_lens);
    if (!p.inside()) return;               // (the lattice walk and the gradient never use these entries)
    const TL* r = logits + row * ldv;
    float M, s;
    row_lse<TL>(r, V, vec_ok, lane, M, s);
    float x[TDT_MAXD];
    const float ldur = tdt_dur_lse<TL>(r + V, D, x);
    if (lane < D) {
        float v = -INFINITY;
#pragma unroll
        for (int j = 0; j < TDT_MAXD; ++j) v = (j == lane) ? x[j] : v;
        v -= ldur;
        ld[(long)lane * rows + row] = v < NEG ? NEG : v;
    }
    if (lane == 0) {
        const float l = M + __logf(s);
        lse_tok[row] = l;
        lse_dur[row] = ldur;
        // clamped at NEG so that a -inf logit is a dead transition and not an inf - inf in the log-add-exp (a NaN stays a NaN)
        const float pb = ldf<TL>(r + blank) - l;
        lpb[row] = pb < NEG ? NEG : pb;
        float pl = NEG;
        if (p.u < p.Ub) {
            const int y = clampi(labels[(long)p.b * (U1 - 1) + p.u], 0, V - 1);
            pl = ldf<TL>(r + y) - l;
            pl = pl < NEG ? NEG : pl;
        }
        lpl[row] = pl;
    }
}

// ------------------------------------------------------------------ alpha / beta
// R = slots per lane (64 R >= U1), PF = emission frames per prefetch chunk, DP = duration planes held per frame (D rounded up to 1, 2, 4, 8)
template <int R, int PF, int DP>
struct TdtRows {
    float pb[PF][R];
    float pl[PF][R];
    float ld[PF][DP][R];
};

// frames f0, f0 + dir, ... (clamped to [0, Tb - 1]) and planes min(j, D - 1): the loads past the utterance's end and behind the last duration
// are unconditional and never used
template <int R, int PF, int DP>
__device__ __forceinline__ void tdt_load_rows(TdtRows<R, PF, DP>& buf, const float* __restrict__ lpb, const float* __restrict__ lpl,
                                              const float* __restrict__ ld, long plane, int D, int f0, int dir, int Tb, int U1, int lane) {
#pragma unroll
    for (int s = 0; s < PF; ++s) {
        const int t = clampi(f0 + dir * s, 0, Tb - 1);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int uc = min(r * 64 + lane, U1 - 1);         // in-range column for the lanes that pad the last slot
            const long o = (long)t * U1 + uc;
            buf.pb[s][r] = lpb[o];
            buf.pl[s][r] = lpl[o];
#pragma unroll
            for (int j = 0; j < DP; ++j) buf.ld[s][j][r] = ld[(long)min(j, D - 1) * plane + o];
        }
    }
}

template <int R, int PF, int DP>
__global__ __launch_bounds__(64) void tdt_alphabeta_kernel(const float* __restrict__ lpb_g, const float* __restrict__ lpl_g,
                                                           const float* __restrict__ ld_g, long plane, const int* __restrict__ act_lens,
                                                           const int* __restrict__ label_lens, int T, int U1, TdtDur dur,
                                                           acc_t* __restrict__ alpha_g, acc_t* __restrict__ beta_g, acc_t* __restrict__ ll,
                                                           float* __restrict__ costs) {
    __shared__ acc_t ring[TDT_MAXD][R * 64];                    // row of frame f: ring[f & 7]; lane l touches columns 64 r + l only
    const int b = blockIdx.x >> 1;
    const bool do_beta = blockIdx.x & 1;
    const int lane = threadIdx.x;
    const int D = dur.n;
    const int Tb = clampi(act_lens[b], 1, T), Ub = clampi(label_lens[b], 0, U1 - 1);
    const float* lpb = lpb_g + (long)b * T * U1;
    const float* lpl = lpl_g + (long)b * T * U1;
    const float* ld = ld_g + (long)b * T * U1;
    acc_t* out = (do_beta ? beta_g : alpha_g) + (long)b * (T + 1) * U1;
    bool vb[R], vl[R], wr[R];              // this slot's cell exists / has a label move / is inside the stored row
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int u = r * 64 + lane;
        vb[r] = u <= Ub;
        vl[r] = u < Ub;
        wr[r] = u < U1;
    }
#pragma unroll
    for (int k = 0; k < TDT_MAXD; ++k)
#pragma unroll
        for (int r = 0; r < R; ++r) ring[k][r * 64 + lane] = (acc_t)NEG;
    TdtRows<R, PF, DP> cur, nxt;
    if (!do_beta) {
        // push: alpha(s, .) is complete when frame s is reached (every move into it left an earlier frame).  Its move of duration d_j adds
        //   lae(alpha(s,u) + lpb(s,u) + ld_j(s,u), alpha(s,u-1) + lpl(s,u-1) + ld_j(s,u-1))   into the pending row s + d_j,
        // the label term formed by its owner (u-1) and rotated.  A move with s + d_j > T_b does not exist.
        ring[0][lane] = (lane == 0) ? 0.0 : (acc_t)NEG;
        tdt_load_rows<R, PF, DP>(cur, lpb, lpl, ld, plane, D, 0, 1, Tb, U1, lane);
        for (int base = 0; base < Tb; base += PF) {
            tdt_load_rows<R, PF, DP>(nxt, lpb, lpl, ld, plane, D, base + PF, 1, Tb, U1, lane);
#pragma unroll
            for (int s = 0; s < PF; ++s) {
                const int t = base + s;
                if (t < Tb) {              // wave-uniform
                    acc_t a[R];
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const int c = r * 64 + lane;
                        a[r] = vb[r] ? ring[t & 7][c] : (acc_t)NEG;
                        ring[t & 7][c] = (acc_t)NEG;            // the row of frame t + 8 from here on
                        if (wr[r]) out[(long)t * U1 + c] = a[r];
                    }
#pragma unroll
                    for (int j = 0; j < DP; ++j) {
                        if (j < D && t + dur.d[j] <= Tb) {      // wave-uniform; no load below it
                            const int k = (t + dur.d[j]) & 7;
                            acc_t x[R];
#pragma unroll
                            for (int r = 0; r < R; ++r)
                                x[r] = rot_r1(vl[r] ? a[r] + (acc_t)cur.pl[s][r] + (acc_t)cur.ld[s][j][r] : (acc_t)NEG);
#pragma unroll
                            for (int r = 0; r < R; ++r) {
                                // lane 0 of slot r: the wrapped lane 63 of slot r-1 (label 64 r - 1); nothing left of label 0
                                const acc_t left = (lane == 0) ? (r > 0 ? x[r > 0 ? r - 1 : 0] : (acc_t)NEG) : x[r];
                                const acc_t term = lae(a[r] + (acc_t)cur.pb[s][r] + (acc_t)cur.ld[s][j][r], left);
                                const int c = r * 64 + lane;
                                ring[k][c] = vb[r] ? lae(ring[k][c], term) : (acc_t)NEG;
                            }
                        }
                    }
                }
            }
#pragma unroll
            for (int s = 0; s < PF; ++s)
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    cur.pb[s][r] = nxt.pb[s][r];
                    cur.pl[s][r] = nxt.pl[s][r];
#pragma unroll
                    for (int j = 0; j < DP; ++j) cur.ld[s][j][r] = nxt.ld[s][j][r];
                }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int c = r * 64 + lane;
            const acc_t a = vb[r] ? ring[Tb & 7][c] : (acc_t)NEG;
            if (wr[r]) out[(long)Tb * U1 + c] = a;
            if (c == Ub) {
                ll[b] = a;
                costs[b] = a <= TDT_DEAD ? INFINITY : (float)(-a);      // no path lands on (T_b, U_b): +inf (a NaN stays a NaN)
            }
        }
    } else {
        // pull: beta(t,u) = lae over j with t + d_j <= T_b of lpb + ld_j + beta(t+d_j, u) and lpl + ld_j + beta(t+d_j, u+1), j ascending
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int c = r * 64 + lane;
            const acc_t v = (c == Ub) ? 0.0 : (acc_t)NEG;
            ring[Tb & 7][c] = v;
            if (wr[r]) out[(long)Tb * U1 + c] = v;
        }
        tdt_load_rows<R, PF, DP>(cur, lpb, lpl, ld, plane, D, Tb - 1, -1, Tb, U1, lane);
        for (int base = Tb - 1; base >= 0; base -= PF) {
            tdt_load_rows<R, PF, DP>(nxt, lpb, lpl, ld, plane, D, base - PF, -1, Tb, U1, lane);
#pragma unroll
            for (int s = 0; s < PF; ++s) {
                const int t = base - s;
                if (t >= 0) {              // wave-uniform
                    acc_t acc[R];
#pragma unroll
                    for (int r = 0; r < R; ++r) acc[r] = (acc_t)NEG;
#pragma unroll
                    for (int j = 0; j < DP; ++j) {
                        if (j < D && t + dur.d[j] <= Tb) {      // wave-uniform; no load below it
                            const int k = (t + dur.d[j]) & 7;
                            acc_t bt[R], x[R];
#pragma unroll
                            for (int r = 0; r < R; ++r) {
                                bt[r] = ring[k][r * 64 + lane];
                                x[r] = rot_l1(bt[r]);
                            }
#pragma unroll
                            for (int r = 0; r < R; ++r) {
                                // lane 63 of slot r: the wrapped lane 0 of slot r+1 (label 64 (r + 1)); nothing right of the last slot
                                const acc_t right = (lane == 63) ? (r + 1 < R ? x[r + 1 < R ? r + 1 : r] : (acc_t)NEG) : x[r];
                                const acc_t tl = vl[r] ? right + (acc_t)cur.pl[s][r] + (acc_t)cur.ld[s][j][r] : (acc_t)NEG;
                                acc[r] = lae(acc[r], lae(bt[r] + (acc_t)cur.pb[s][r] + (acc_t)cur.ld[s][j][r], tl));
                            }
                        }
                    }
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        const int c = r * 64 + lane;
                        acc[r] = vb[r] ? acc[r] : (acc_t)NEG;
                        ring[t & 7][c] = acc[r];                // frame t + 8 is behind every later pull
                        if (wr[r]) out[(long)t * U1 + c] = acc[r];
                    }
                }
            }
#pragma unroll
            for (int s = 0; s < PF; ++s)
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    cur.pb[s][r] = nxt.pb[s][r];
                    cur.pl[s][r] = nxt.pl[s][r];
#pragma unroll
                    for (int j = 0; j < DP; ++j) cur.ld[s][j][r] = nxt.ld[s][j][r];
                }
        }
    }
}

// ------------------------------------------------------------------ gradient
template <typename TL>
__global__ __launch_bounds__(TDT_WAVES * 64) void tdt_grad_kernel(
    const TL* logits, long ldv, const int* __restrict__ labels, const int* __restrict__ act_lens, const int* __restrict__ label_lens,
    int B, int T, int U1, int V, TdtDur dur, int blank, int vec_ok, const float* __restrict__ lse_tok, const float* __restrict__ lse_dur,
    const acc_t* __restrict__ alpha_g, const acc_t* __restrict__ beta_g, const acc_t* __restrict__ ll, const float* __restrict__ grad_out,
    int grad_out_stride, float scale, TL* grad, long ldg) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * TDT_WAVES + (threadIdx.x >> 6);
    if (row >= (long)B * T * U1) return;
    const int D = dur.n;
    const LatticeRow p = lattice_row(row, T, U1, act_lens, label_lens);
    const int b = p.b, t = p.t, u = p.u, Ub = p.Ub, Tb = p.Tb;
    const acc_t L = ll[b];
    // rows outside the lattice and utterances without a path: zero rows
    const bool valid = p.inside() && !(L <= TDT_DEAD);
    const TL* r = logits + row * ldv;
    float c = 0.f, cd = 0.f, eb = 0.f, el = 0.f, gs = 0.f, gd = 0.f;
    int yv = -1;
    if (valid) {
        const long ai = ((long)b * (T + 1) + t) * U1 + u;                       // (t, u); (t + d, u) is d * U1 further
        const float l = lse_tok[row], lq = lse_dur[row];
        const acc_t a = alpha_g[ai] - L;                                        // alpha - ll, fp64
        const float occ = (float)(a + beta_g[ai]);
        c = occ - l;
        cd = occ - lq;
        gs = scale * grad_out[(long)b * grad_out_stride];
        float x[TDT_MAXD];
        tdt_dur_lse<TL>(r + V, D, x);
        const float lpb = ldf<TL>(r + blank) - l;
        float lpy = NEG;
        if (u < Ub) {
            yv = clampi(labels[(long)b * (U1 - 1) + u], 0, V - 1);
            lpy = ldf<TL>(r + yv) - l;
        }
        const int un = min(u + 1, U1 - 1);                                      // beta(., u + 1): clamped, dropped by the select for u = U_b
#pragma unroll
        for (int j = 0; j < TDT_MAXD; ++j) {
            const int d = dur.d[j];
            const bool mv = j < D && t + d <= Tb;                               // the move exists
            const long bi = ((long)b * (T + 1) + min(t + d, Tb)) * U1;
            const float ldj = x[j] - lq;
            const float ebj = mv ? __expf((float)(a + beta_g[bi + u]) + lpb + ldj) : 0.f;
            const float elj = (mv && u < Ub) ? __expf((float)(a + beta_g[bi + un]) + lpy + ldj) : 0.f;
            eb += ebj;
            el += elj;
            // d z[V + j] = g (softmax_dur[j] occ - E_j): lane j keeps column V + j
            const float g = (j < D) ? gs * (__expf(x[j] + cd) - (ebj + elj)) : 0.f;
            gd = (lane == j) ? g : gd;
        }
    }
    // every lane has read r[blank], r[yv] and the duration columns before any lane overwrites them (in-place use)
    __builtin_amdgcn_wave_barrier();
    TL* g = grad + row * ldg;
    row_map<TL>(r, g, V, V, vec_ok, lane, valid, [&](float x, int v) -> float {
        float e = __expf(x + c);
        e -= (v == blank) ? eb : 0.f;
        e -= (v == yv) ? el : 0.f;
        return valid ? gs * e : 0.f;
    });
    if (lane < D) stf<TL>(g + V + lane, valid ? gd : 0.f);
    for (long i = V + D + lane; i < ldg; i += 64) stf<TL>(g + i, 0.f);
}

// ------------------------------------------------------------------ greedy decode
// One wave per row (b, r) of the block: dec[row] = (k*, j*), lp[row] = (lt[k*], ld[j*]); rows of utterances that do not need a symbol and
// frames that do not exist are left alone.  Token sub-row: the single pass of greedy_scan_batch_lp_kernel (argmax order of rowops.h: the
// lowest index wins a tie, a NaN counts as the largest value).  Duration sub-row: D <= 8 values in registers, the same order.
template <typename TL>
__global__ __launch_bounds__(256) void tdt_scan_kernel(const TL* __restrict__ logits, long ld, int B, int n, int V, int D,
                                                       const int* __restrict__ t, const int* __restrict__ T_len, const int* __restrict__ need,
                                                       int* __restrict__ dec, float* __restrict__ lp) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= B * n) return;
    const int b = row / n, r = row - b * n;
    if (!need[b] || t[b] + r >= T_len[b]) return;       // (wave-uniform)
    const TL* p = logits + (long)row * ld;
    float best = -INFINITY, m = -INFINITY, s = 0.f;
    int bi = 0x7fffffff;
    for (int v = lane; v < V; v += 64) {
        const float x = ldf<TL>(p + v);
        if (argmax_takes(x, v, best, bi)) { best = x; bi = v; }
        if (x != -INFINITY) {                            // (-inf against m = -inf would be exp(NaN))
            const float e = __expf(-fabsf(x - m));
            if (x > m) { s = s * e + 1.f; m = x; }
            else s += e;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        const float om = __shfl_xor(m, o, 64), os = __shfl_xor(s, o, 64);
        if (argmax_takes(ob, oi, best, bi)) { best = ob; bi = oi; }
        const float nm = fmaxf(m, om);
        s = s * (m == nm ? 1.f : __expf(m - nm)) + os * (om == nm ? 1.f : __expf(om - nm));
        m = nm;
    }
    if (lane == 0) {
        float dbest = -INFINITY, dm = -INFINITY;
        int dj = 0x7fffffff;
        float x[TDT_MAXD];
#pragma unroll
        for (int j = 0; j < TDT_MAXD; ++j) {
            x[j] = ldf<TL>(p + V + (j < D ? j : D - 1));
            if (j < D) {
                if (argmax_takes(x[j], j, dbest, dj)) { dbest = x[j]; dj = j; }
                dm = fmaxf(dm, x[j]);
            }
        }
        float ds = 0.f;
#pragma unroll
        for (int j = 0; j < TDT_MAXD; ++j) ds += (j < D && x[j] != -INFINITY) ? __expf(x[j] - dm) : 0.f;
        const float lse = m + logf(s), dlse = dm + logf(ds);
        dec[2 * (long)row] = bi;
        dec[2 * (long)row + 1] = dj;
        lp[2 * (long)row] = (lse - lse == 0.f) ? best - lse : NAN;
        lp[2 * (long)row + 1] = (dlse - dlse == 0.f) ? dbest - dlse : NAN;
    }
}

// One thread per utterance with need[b]: follow the jumps through the block from row 0.  A decision at row r (frame t0 + r, which exists and
// lies inside the block) adds lt + ld to the f64 score and moves r on by its duration; a token is booked and ends the walk.  A jump that
// leaves the block carries over: t = t0 + r exactly.  flags[0] = utterances that still need a symbol, flags[1] = utterances not finished,
// counted in LDS by the one workgroup and written (not added): nothing has to be zeroed before the call.
__global__ __launch_bounds__(256) void tdt_advance_kernel(const int* __restrict__ dec, const float* __restrict__ lp, int B, int n, int blank,
                                                          TdtDur dur, int n_hist, long* __restrict__ hist, long ld_hist, int* __restrict__ t,
                                                          const int* __restrict__ T_len, int* __restrict__ need, int* __restrict__ done,
                                                          int* __restrict__ count, int* __restrict__ flags, int* __restrict__ frames,
                                                          float* __restrict__ tok_lp, int* __restrict__ tok_dur, long ld_det,
                                                          double* __restrict__ score) {
    __shared__ int f[2];
    if (threadIdx.x < 2) f[threadIdx.x] = 0;
    __syncthreads();
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        if (need[b]) {
            const int t0 = t[b], Tl = T_len[b];
            double sc = score[b];
            int r = 0;
            while (r < n && t0 + r < Tl) {
                const long row = (long)b * n + r;
                const int k = dec[2 * row], d = dur.d[clampi(dec[2 * row + 1], 0, dur.n - 1)];
                sc += (double)lp[2 * row] + (double)lp[2 * row + 1];
                r += d;
                if (k != blank) {
                    const int c = count[b];
                    if (c < ld_det) {                              // (the contract asks for it; never write past the row)
                        frames[(long)b * ld_det + c] = t0 + r - d;
                        tok_lp[(long)b * ld_det + c] = lp[2 * row];
                        tok_dur[(long)b * ld_det + c] = d;
                    }
                    hist[(long)b * ld_hist + n_hist] = (long)k;
                    count[b] = c + 1;
                    need[b] = 0;
                    break;
                }
            }
            score[b] = sc;
            t[b] = t0 + r;
            if (t0 + r >= Tl) { need[b] = 0; done[b] = 1; }
        }
        if (need[b]) atomicAdd(&f[0], 1);
        if (!done[b]) atomicAdd(&f[1], 1);
    }
    __syncthreads();
    if (threadIdx.x < 2) flags[threadIdx.x] = f[threadIdx.x];
}

// durations: a HOST array of D entries, distinct integers in [1, 8] in strictly increasing order
int tdt_durations(const char* who, const int* durations, int D, TdtDur& dur) {
    TTMI_REQUIRE(durations, "%s: null pointer", who);
    TTMI_REQUIRE(D >= 1 && D <= TDT_MAXD, "%s: D=%d outside [1,%d]", who, D, TDT_MAXD);
    for (int j = 0; j < TDT_MAXD; ++j) dur.d[j] = 0;
    dur.n = D;
    for (int j = 0; j < D; ++j) {
        TTMI_REQUIRE(durations[j] >= 1 && durations[j] <= TDT_MAXD, "%s: duration %d outside [1,%d]", who, durations[j], TDT_MAXD);
        TTMI_REQUIRE(j == 0 || durations[j] > durations[j - 1], "%s: durations must be strictly increasing", who);
        dur.d[j] = durations[j];
    }
    return TTMI_OK;
}

// fn(DP) with DP = D rounded up to 1, 2, 4 or 8, a std::integral_constant
template <typename Fn>
void with_planes(int D, Fn&& fn) {
    using std::integral_constant;
    if (D <= 1) fn(integral_constant<int, 1>{});
    else if (D <= 2) fn(integral_constant<int, 2>{});
    else if (D <= 4) fn(integral_constant<int, 4>{});
    else fn(integral_constant<int, 8>{});
}

}  // namespace

extern "C" {

// bytes of caller-provided workspace shared by ttmi_tdt_loss_fwd / _bwd (8-byte aligned)
size_t ttmi_tdt_workspace_bytes(int B, int T, int U1, int D) {
    if (B <= 0 || T <= 0 || U1 <= 0 || D < 1 || D > TDT_MAXD) return 0;
    return sizeof(acc_t) * (2 * (size_t)B * (T + 1) * U1 + (size_t)B) + sizeof(float) * (4 + (size_t)D) * (size_t)B * T * U1 + 64;
}

int ttmi_tdt_loss_fwd(const void* logits, int dtype, long ldv, const int* labels, const int* act_lens, const int* label_lens, int B, int T,
                      int U1, int V, int blank, const int* durations, int D, void* workspace, float* costs, void* stream) {
    TTMI_REQUIRE(logits && (labels || U1 == 1) && act_lens && label_lens && workspace && costs, "tdt_loss_fwd: null pointer");
    TTMI_REQUIRE(B > 0 && T > 0 && U1 > 0 && V > 0, "tdt_loss_fwd: bad shape B=%d T=%d U1=%d V=%d", B, T, U1, V);
    TdtDur dur;
    if (int rc = tdt_durations("tdt_loss_fwd", durations, D, dur)) return rc;
    TTMI_REQUIRE(ldv >= (long)V + D && (dtype == 0 || dtype == 1), "tdt_loss_fwd: bad pitch/dtype (ldv must hold V + D columns)");
    TTMI_REQUIRE(blank >= 0 && blank < V, "tdt_loss_fwd: blank %d outside [0,%d)", blank, V);
    TTMI_REQUIRE(U1 <= 1024, "tdt_loss_fwd: U+1=%d > 1024 unsupported", U1);
    TTMI_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "tdt_loss_fwd: workspace must be 8-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const TdtWs w = tdt_carve(workspace, B, T, U1);
    const long rows = (long)B * T * U1;
    const int vec_ok = rows_vec_ok(logits, dtype == 0 ? 4 : 2);
    by_dtype(dtype, [&](auto z) {
        using TL = decltype(z);
        hipLaunchKernelGGL(tdt_lse_kernel<TL>, dim3(cdiv(rows, TDT_WAVES)), dim3(TDT_WAVES * 64), 0, st, static_cast<const TL*>(logits), ldv,
                           labels, act_lens, label_lens, B, T, U1, V, D, blank, vec_ok, w.lse_tok, w.lse_dur, w.lpb, w.lpl, w.ld);
    });
    TTMI_LAUNCH_CHECK("tdt_lse_kernel");
    with_slots(U1, [&](auto R, auto) {
        with_planes(D, [&](auto DP) {
            // prefetch depth: what the emission tables of one frame ((2 + DP) floats per slot) leave room for
            constexpr int PF = (R * (2 + DP) <= 6) ? 4 : (R * (2 + DP) <= 12 ? 2 : 1);
            hipLaunchKernelGGL((tdt_alphabeta_kernel<R, PF, DP>), dim3(2 * B), dim3(64), 0, st, w.lpb, w.lpl, w.ld, rows, act_lens, label_lens, T,
                               U1, dur, w.alpha, w.beta, w.ll, costs);
        });
    });
    TTMI_LAUNCH_CHECK("tdt_alphabeta_kernel");
    return TTMI_OK;
}

int ttmi_tdt_loss_bwd(const void* logits, int dtype, long ldv, const int* labels, const int* act_lens, const int* label_lens, int B, int T,
                      int U1, int V, int blank, const int* durations, int D, const void* workspace, const float* grad_out,
                      int grad_out_stride, float scale, void* grad, long ldg, void* stream) {
    TTMI_REQUIRE(logits && (labels || U1 == 1) && act_lens && label_lens && workspace && grad_out && grad, "tdt_loss_bwd: null pointer");
    TTMI_REQUIRE(B > 0 && T > 0 && U1 > 0 && V > 0, "tdt_loss_bwd: bad shape B=%d T=%d U1=%d V=%d", B, T, U1, V);
    TdtDur dur;
    if (int rc = tdt_durations("tdt_loss_bwd", durations, D, dur)) return rc;
    TTMI_REQUIRE(ldv >= (long)V + D && ldg >= (long)V + D && (dtype == 0 || dtype == 1),
                 "tdt_loss_bwd: bad pitch/dtype (ldv and ldg must hold V + D columns)");
    TTMI_REQUIRE(blank >= 0 && blank < V, "tdt_loss_bwd: blank %d outside [0,%d)", blank, V);
    TTMI_REQUIRE(U1 <= 1024, "tdt_loss_bwd: U+1=%d > 1024 unsupported", U1);
    TTMI_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7) == 0, "tdt_loss_bwd: workspace must be 8-byte aligned");
    TTMI_REQUIRE(logits != static_cast<const void*>(grad) || ldg == ldv, "tdt_loss_bwd: in-place needs ldg == ldv");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const TdtWs w = tdt_carve(const_cast<void*>(workspace), B, T, U1);
    const long rows = (long)B * T * U1;
    const int vec_ok = rows_vec_ok(logits, grad, ldv, ldg, dtype == 0 ? 4 : 2);
    by_dtype(dtype, [&](auto z) {
        using TL = decltype(z);
        hipLaunchKernelGGL(tdt_grad_kernel<TL>, dim3(cdiv(rows, TDT_WAVES)), dim3(TDT_WAVES * 64), 0, st, static_cast<const TL*>(logits), ldv,
                           labels, act_lens, label_lens, B, T, U1, V, dur, blank, vec_ok, w.lse_tok, w.lse_dur, w.alpha, w.beta, w.ll, grad_out,
                           grad_out_stride, scale, static_cast<TL*>(grad), ldg);
    });
    TTMI_LAUNCH_CHECK("tdt_grad_kernel");
    return TTMI_OK;
}

int ttmi_tdt_scan_batch(const void* logits, int dtype, long ld, int B, int n, int V, int D, const int* t, const int* T_len, const int* need,
                        int* dec, float* lp, void* stream) {
    TTMI_REQUIRE(logits && t && T_len && need && dec && lp, "tdt_scan_batch: null pointer");
    TTMI_REQUIRE(B > 0 && n > 0 && V > 0 && (long)B * n < (1L << 30), "tdt_scan_batch: bad shape B=%d n=%d V=%d", B, n, V);
    TTMI_REQUIRE(D >= 1 && D <= TDT_MAXD, "tdt_scan_batch: D=%d outside [1,%d]", D, TDT_MAXD);
    TTMI_REQUIRE(ld >= (long)V + D && (dtype == 0 || dtype == 1), "tdt_scan_batch: bad pitch/dtype (ld must hold V + D columns)");
    hipStream_t st = static_cast<hipStream_t>(stream);
    by_dtype(dtype, [&](auto z) {
        using TL = decltype(z);
        hipLaunchKernelGGL(tdt_scan_kernel<TL>, dim3(cdiv((long)B * n, 4)), dim3(256), 0, st, static_cast<const TL*>(logits), ld, B, n, V, D, t,
                           T_len, need, dec, lp);
    });
    TTMI_LAUNCH_CHECK("tdt_scan_kernel");
    return TTMI_OK;
}

int ttmi_tdt_advance(const int* dec, const float* lp, int B, int n, int blank, const int* durations, int D, int n_hist, long* hist,
                     long ld_hist, int* t, const int* T_len, int* need, int* done, int* count, int* flags, int* frames, float* tok_lp,
                     int* tok_dur, long ld_det, double* score, void* stream) {
    TTMI_REQUIRE(dec && lp && hist && t && T_len && need && done && count && flags && frames && tok_lp && tok_dur && score,
                 "tdt_advance: null pointer");
    TdtDur dur;
    if (int rc = tdt_durations("tdt_advance", durations, D, dur)) return rc;
    TTMI_REQUIRE(B > 0 && n > 0 && n_hist >= 1 && n_hist < ld_hist && ld_det > 0, "tdt_advance: bad arguments");
    hipLaunchKernelGGL(tdt_advance_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), dec, lp, B, n, blank, dur, n_hist, hist,
                       ld_hist, t, T_len, need, done, count, flags, frames, tok_lp, tok_dur, ld_det, score);
    TTMI_LAUNCH_CHECK("tdt_advance_kernel");
    return TTMI_OK;
}

}  // extern "C"
