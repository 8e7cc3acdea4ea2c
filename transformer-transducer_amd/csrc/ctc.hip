// CTC loss on the audio encoder's auxiliary head, and its greedy decode, for gfx950 (no reference counterpart: the reference trains the
// transducer loss alone).
//
//   ctc_link_kernel       per utterance: which label positions carry the same symbol (a chain from the first occurrence through the
//                         later ones), so that the gradient's sum over the states of one symbol has ONE owner and a fixed order.
//   ctc_lse_kernel        HBM-bound: one wave per (b,t) row of V logits, lattice.h's row_lse walk; gathers
//                         lp(t, s) = log_softmax(z[b,t])[l'_s] for the 2 U_b + 1 states of the extended label sequence.
//   ctc_alphabeta_kernel  latency-bound dynamic programme: one workgroup per (utterance, direction), ONE launch for all T frames.  Thread
//                         k owns the state pair (2k, 2k+1) = (blank before label k, label k): the s-1 neighbour of the label state is the
//                         thread's own blank state, and the s-1 / s-2 neighbours that live elsewhere are both "label k-1", which arrives
//                         by a one-lane DPP wave rotate (beta: the pair of thread k+1, two rotates).  U + 1 <= 64 (the training
//                         workload's U = 50) is one wave with no barrier in the walk; longer label sequences are several waves, the
//                         cell that crosses a wave boundary goes through a double-buffered LDS slot, one barrier per frame.  Emission
//                         rows are prefetched CTC_PF frames ahead into registers.  Frontier in fp64 (lattice.h: lae).
//   ctc_score_kernel      the alpha walk alone for P (hypothesis, utterance) pairs (ttmi_ctc_score_hyps: N-best rescoring): no emission table,
//                         no stored alpha; every thread gathers its symbol's logit CTC_PF frames ahead, the log-sum-exp comes from
//                         ctc_lse_kernel<false> once per utterance.
//   ctc_grad_kernel       HBM-bound: one wave per row reads the logits once and writes g * softmax once (in place allowed), then the
//                         owners of the row's symbols overwrite their columns with g * (softmax - occupancy).  No atomics.
//   ctc_greedy_kernel     per-frame argmax in the order of the transducer's greedy scans (rowops.h), repeats collapsed, blanks dropped.
#include "common.h"
#include "lattice.h"
#include "rowops.h"

namespace {

using namespace ttmi_lattice;

constexpr int CTC_ROW_WAVES = 4;
constexpr int CTC_PF = 8;                 // emission rows in flight per thread of the lattice walk
constexpr acc_t CTC_DEAD = -1e29;         // a log-likelihood below this never met a live path (dead cells sit near NEG = -1e30)
constexpr int LINK_FIRST = 1 << 16;       // link word: bits 0..15 = next position with the same symbol + 1 (0 = none), bit 16 = first occurrence

// states per frame, padded to the pairs the lattice threads own: thread k <= U holds (2k, 2k+1); state 2U+1 is padding
__host__ __device__ __forceinline__ long ctc_sp(int U) { return 2L * (U + 1); }

struct CtcWs {
    acc_t *alpha, *beta, *ll;             // [B, T, Sp] x 2, [B]
    float *lse, *lp;                      // [B, T], [B, T, Sp]
    int* link;                            // [B, U]
};
__host__ __forceinline__ long even(long n) { return (n + 1) & ~1L; }
CtcWs ctc_carve(void* ws, int B, int T, int U) {
    const long n = (long)B * T * ctc_sp(U);
    CtcWs w;
    acc_t* q = static_cast<acc_t*>(ws);   // fp64 part first: the pairs are stored as 16-byte granules (workspace 16-byte aligned, Sp even)
    w.alpha = q; q += n;
    w.beta = q; q += n;
    w.ll = q; q += even(B);
    float* p = reinterpret_cast<float*>(q);
    w.lse = p; p += even((long)B * T);
    w.lp = p; p += n;
    w.link = reinterpret_cast<int*>(p);
    return w;
}

// ------------------------------------------------------------------ symbol chains
__global__ __launch_bounds__(256) void ctc_link_kernel(const int* __restrict__ labels, const int* __restrict__ label_lens, int U, int V,
                                                       int blank, int* __restrict__ link) {
    __shared__ int y[1024];
    const int b = blockIdx.x;
    const int Ub = clampi(label_lens[b], 0, U);
    for (int u = threadIdx.x; u < Ub; u += 256) y[u] = clampi(labels[(long)b * U + u], 0, V - 1);
    __syncthreads();
    for (int u = threadIdx.x; u < Ub; u += 256) {
        int w = 0;
        if (y[u] != blank) {               // a label equal to `blank` is one more blank state: the blank column's owner (lane 0) sums it
            bool first = true;
            for (int j = 0; j < u; ++j) first = first && (y[j] != y[u]);
            int nxt = -1;
            for (int j = Ub - 1; j > u; --j) nxt = (y[j] == y[u]) ? j : nxt;
            w = (nxt + 1) | (first ? LINK_FIRST : 0);
        }
        link[(long)b * U + u] = w;
    }
}

// lp(t, s) from the symbol's logit and the row's log-sum-exp; clamped at NEG so that a -inf logit is a dead transition and not an inf - inf
// in the log-add-exp (a NaN stays a NaN)
__device__ __forceinline__ float ctc_emit(float z, float lse) {
    const float v = z - lse;
    return v < NEG ? NEG : v;
}

// ------------------------------------------------------------------ lse + gather
// GATHER = false (ttmi_ctc_score_hyps): the log-sum-exp alone - labels, label_lens and lp are not touched
template <bool GATHER>
__global__ __launch_bounds__(CTC_ROW_WAVES * 64) void ctc_lse_kernel(
    const float* __restrict__ logits, long ldv, const int* __restrict__ labels, const int* __restrict__ act_lens,
    const int* __restrict__ label_lens, int B, int T, int U, int V, int blank, int vec_ok, float* __restrict__ lse,
    float* __restrict__ lp) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * CTC_ROW_WAVES + (threadIdx.x >> 6);
    if (row >= (long)B * T) return;
    const int t = (int)(row % T);
    const int b = (int)(row / T);
    const int Tb = clampi(act_lens[b], 1, T);
    if (t >= Tb) return;
    const float* r = logits + row * ldv;
    float M, s;
    row_lse<float>(r, V, vec_ok, lane, M, s);
    const float l = M + __logf(s);
    if (lane == 0) lse[row] = l;
    if constexpr (GATHER) {
        // the row's 2 U_b + 1 emission log-probs (the row is in cache: it has just been read)
        const int Ub = clampi(label_lens[b], 0, U);
        float* lpr = lp + row * ctc_sp(U);
        const int S = 2 * Ub + 1;
        for (int si = lane; si < S; si += 64) {
            const int sym = (si & 1) ? clampi(labels[(long)b * U + (si >> 1)], 0, V - 1) : blank;
            lpr[si] = ctc_emit(r[sym], l);
        }
    }
}

// ------------------------------------------------------------------ hypothesis scorer: the alpha walk alone, emissions gathered from the logits
// score[p] = log P_ctc(hyp[p] | logits[utt(p)]): the alpha half of ctc_alphabeta_kernel, term for term and in its order, in the same shape
// (thread k owns the state pair (2k, 2k+1), "label k-1" by the one-lane DPP rotate, the double-buffered LDS slot across a wave boundary;
// U + 1 <= 64: one wave, no barrier in the walk) - without the emission table and without storing alpha.  Each thread gathers its own
// symbol's logit z[b, t, y_k] CTC_PF frames ahead; the blank column and lse[b, t] are the same address for the whole workgroup.  The pairs of
// one utterance are neighbours in the grid: after its first hypothesis the utterance's rows come from cache.
template <bool MULTI>
__global__ __launch_bounds__(MULTI ? 1024 : 64) void ctc_score_kernel(
    const float* __restrict__ logits, long ldv, const float* __restrict__ lse, const int* __restrict__ act_lens, int B, int T, int V,
    int blank, const long* __restrict__ hyp, long ld_hyp, const int* __restrict__ hyp_len, const int* __restrict__ utt, int per, int U,
    acc_t* __restrict__ score) {
    __shared__ acc_t bnd[2][16];          // the label cell that crosses a wave boundary, double-buffered by frame parity
    __shared__ acc_t fin;
    const int p = blockIdx.x;
    const int b = utt ? clampi(utt[p], 0, B - 1) : p / per;     // utt == NULL: P = B * per, the beam's [B, W] layout
    const int k = threadIdx.x, lane = k & 63, wave = k >> 6;
    const int Tb = clampi(act_lens[b], 1, T), Ub = clampi(hyp_len[p], 0, U);
    const bool vb = k <= Ub, vl = k < Ub;             // this thread's blank / label state exists
    const long* h = hyp + (long)p * ld_hyp;
    auto tok = [&](int i) -> int {
        const long v = h[i];
        return (int)(v < 0 ? 0 : (v > V - 1 ? V - 1 : v));
    };
    const int yk = vl ? tok(k) : -1;
    // skip transition into label state 2k+1 from 2k-1: l'_s != blank and l'_s != l'_{s-2}
    const bool skip = vl && k > 0 && yk != blank && yk != tok(k > 0 ? k - 1 : 0);
    const float* zr = logits + (long)b * T * ldv;
    const float* ls = lse + (long)b * T;
    const int col = vl ? yk : blank;                  // threads without a label state gather the blank column (in range, never used)
    struct Em { float zb, zl, l; };                   // frame t as loaded: blank logit, own symbol's logit, log-sum-exp
    auto load = [&](int t) -> Em { return Em{zr[(long)t * ldv + blank], zr[(long)t * ldv + col], ls[t]}; };
    Em cur[CTC_PF], nxt[CTC_PF];
    const Em e0 = load(0);
    acc_t ab = k == 0 ? (acc_t)ctc_emit(e0.zb, e0.l) : (acc_t)NEG;
    acc_t al = (k == 0 && vl) ? (acc_t)ctc_emit(e0.zl, e0.l) : (acc_t)NEG;
#pragma unroll
    for (int i = 0; i < CTC_PF; ++i) cur[i] = load(min(1 + i, Tb - 1));
    for (int base = 1; base < Tb; base += CTC_PF) {
#pragma unroll
        for (int i = 0; i < CTC_PF; ++i) nxt[i] = load(min(base + CTC_PF + i, Tb - 1));
#pragma unroll
        for (int i = 0; i < CTC_PF; ++i) {
            const int t = base + i;
            if (t < Tb) {                              // workgroup-uniform
                if (MULTI) {
                    if (lane == 63) bnd[t & 1][wave] = al;
                    __syncthreads();
                }
                acc_t nb = rot_r1(al);                 // label state of thread k-1 at frame t-1
                if (lane == 0) nb = (MULTI && wave > 0) ? bnd[t & 1][wave > 0 ? wave - 1 : 0] : (acc_t)NEG;
                acc_t ml = lae(al, ab);
                if (skip) ml = lae(ml, nb);
                const acc_t nab = vb ? (acc_t)ctc_emit(cur[i].zb, cur[i].l) + lae(ab, nb) : (acc_t)NEG;
                al = vl ? (acc_t)ctc_emit(cur[i].zl, cur[i].l) + ml : (acc_t)NEG;
                ab = nab;
            }
        }
#pragma unroll
        for (int i = 0; i < CTC_PF; ++i) cur[i] = nxt[i];
    }
    // logsumexp(alpha(T_b-1, 2 U_b), alpha(T_b-1, 2 U_b - 1)): thread U_b holds the first, thread U_b - 1 the second
    if (Ub > 0 && k == Ub - 1) fin = al;
    __syncthreads();
    if (k == Ub) {
        const acc_t v = Ub > 0 ? lae(ab, fin) : ab;
        score[p] = v <= CTC_DEAD ? (acc_t)-INFINITY : v;            // no feasible alignment: -inf, the loss's +inf (a NaN stays a NaN)
    }
}

// ------------------------------------------------------------------ alpha / beta
template <bool MULTI>
__global__ __launch_bounds__(MULTI ? 1024 : 64) void ctc_alphabeta_kernel(
    const float* __restrict__ lp, const int* __restrict__ labels, const int* __restrict__ act_lens, const int* __restrict__ label_lens,
    int T, int U, int V, int blank, acc_t* __restrict__ alpha, acc_t* __restrict__ beta, acc_t* __restrict__ ll,
    float* __restrict__ costs) {
    __shared__ acc_t bnd[2][16][2];       // the cells that cross a wave boundary, double-buffered by frame parity
    __shared__ acc_t fin;
    const int b = blockIdx.x >> 1;
    const bool do_beta = blockIdx.x & 1;
    const int k = threadIdx.x, lane = k & 63, wave = k >> 6, W = blockDim.x >> 6;
    const int Tb = clampi(act_lens[b], 1, T), Ub = clampi(label_lens[b], 0, U);
    const bool vb = k <= Ub, vl = k < Ub;             // this thread's blank / label state exists
    const int* lab = labels + (long)b * U;
    const int yk = vl ? clampi(lab[k], 0, V - 1) : -1;
    const long rp = ctc_sp(U) / 2;                    // pairs per frame
    const int kc = k <= U ? k : U;                    // in-range pair for the (unconditional) loads of the threads that pad the last wave
    const float2* e2 = reinterpret_cast<const float2*>(lp + (long)b * T * ctc_sp(U)) + kc;
    double2* out = reinterpret_cast<double2*>((do_beta ? beta : alpha) + (long)b * T * ctc_sp(U)) + kc;
    const bool wr = k <= U;
    float2 cur[CTC_PF], nxt[CTC_PF];
    if (!do_beta) {
        // skip transition into label state 2k+1 from 2k-1: l'_s != blank and l'_s != l'_{s-2}
        const bool skip = vl && k > 0 && yk != blank && yk != clampi(lab[k > 0 ? k - 1 : 0], 0, V - 1);
        const float2 e0 = e2[0];
        acc_t ab = k == 0 ? (acc_t)e0.x : (acc_t)NEG;
        acc_t al = (k == 0 && vl) ? (acc_t)e0.y : (acc_t)NEG;
        if (wr) out[0] = make_double2(ab, al);
#pragma unroll
        for (int i = 0; i < CTC_PF; ++i) cur[i] = e2[(long)min(1 + i, Tb - 1) * rp];
        for (int base = 1; base < Tb; base += CTC_PF) {
#pragma unroll
            for (int i = 0; i < CTC_PF; ++i) nxt[i] = e2[(long)min(base + CTC_PF + i, Tb - 1) * rp];
#pragma unroll
            for (int i = 0; i < CTC_PF; ++i) {
                const int t = base + i;
                if (t < Tb) {                          // workgroup-uniform
                    if (MULTI) {
                        if (lane == 63) bnd[t & 1][wave][0] = al;
                        __syncthreads();
                    }
                    acc_t nb = rot_r1(al);             // label state of thread k-1 at frame t-1
                    if (lane == 0) nb = (MULTI && wave > 0) ? bnd[t & 1][wave > 0 ? wave - 1 : 0][0] : (acc_t)NEG;
                    acc_t ml = lae(al, ab);
                    if (skip) ml = lae(ml, nb);
                    const acc_t nab = vb ? (acc_t)cur[i].x + lae(ab, nb) : (acc_t)NEG;
                    al = vl ? (acc_t)cur[i].y + ml : (acc_t)NEG;
                    ab = nab;
                    if (wr) out[(long)t * rp] = make_double2(ab, al);
                }
            }
#pragma unroll
            for (int i = 0; i < CTC_PF; ++i) cur[i] = nxt[i];
        }
        // ll = logsumexp(alpha(T_b-1, 2 U_b), alpha(T_b-1, 2 U_b - 1)): thread U_b holds the first, thread U_b - 1 the second
        if (Ub > 0 && k == Ub - 1) fin = al;
        __syncthreads();
        if (k == Ub) {
            const acc_t v = Ub > 0 ? lae(ab, fin) : ab;
            ll[b] = v;
            costs[b] = v <= CTC_DEAD ? INFINITY : (float)(-v);      // no feasible alignment: +inf (a NaN stays a NaN)
        }
    } else {
        // skip transition out of label state 2k+1 into 2k+3: l'_{s+2} != blank and l'_{s+2} != l'_s
        const int yn = (k + 1 < Ub) ? clampi(lab[k + 1 < Ub ? k + 1 : 0], 0, V - 1) : -1;
        const bool skip = (k + 1 < Ub) && yn != blank && yn != yk;
        const float2 e0 = e2[(long)(Tb - 1) * rp];
        acc_t bb = k == Ub ? (acc_t)e0.x : (acc_t)NEG;
        acc_t bl = k == Ub - 1 ? (acc_t)e0.y : (acc_t)NEG;
        if (wr) out[(long)(Tb - 1) * rp] = make_double2(bb, bl);
#pragma unroll
        for (int i = 0; i < CTC_PF; ++i) cur[i] = e2[(long)max(Tb - 2 - i, 0) * rp];
        for (int base = Tb - 2; base >= 0; base -= CTC_PF) {
#pragma unroll
            for (int i = 0; i < CTC_PF; ++i) nxt[i] = e2[(long)max(base - CTC_PF - i, 0) * rp];
#pragma unroll
            for (int i = 0; i < CTC_PF; ++i) {
                const int t = base - i;
                if (t >= 0) {                          // workgroup-uniform
                    if (MULTI) {
                        if (lane == 0) { bnd[t & 1][wave][0] = bb; bnd[t & 1][wave][1] = bl; }
                        __syncthreads();
                    }
                    acc_t nbb = rot_l1(bb), nbl = rot_l1(bl);          // the pair of thread k+1 at frame t+1
                    if (lane == 63) {
                        const bool has = MULTI && wave + 1 < W;
                        nbb = has ? bnd[t & 1][wave + 1 < W ? wave + 1 : wave][0] : (acc_t)NEG;
                        nbl = has ? bnd[t & 1][wave + 1 < W ? wave + 1 : wave][1] : (acc_t)NEG;
                    }
                    acc_t ml = lae(bl, nbb);
                    if (skip) ml = lae(ml, nbl);
                    const acc_t nbbv = vb ? (acc_t)cur[i].x + lae(bb, bl) : (acc_t)NEG;
                    bl = vl ? (acc_t)cur[i].y + ml : (acc_t)NEG;
                    bb = nbbv;
                    if (wr) out[(long)t * rp] = make_double2(bb, bl);
                }
            }
#pragma unroll
            for (int i = 0; i < CTC_PF; ++i) cur[i] = nxt[i];
        }
    }
}

// ------------------------------------------------------------------ gradient
__global__ __launch_bounds__(CTC_ROW_WAVES * 64) void ctc_grad_kernel(
    const float* logits, long ldv, const int* __restrict__ labels, const int* __restrict__ act_lens, const int* __restrict__ label_lens,
    int B, int T, int U, int V, int blank, int vec_ok, const float* __restrict__ lse, const float* __restrict__ lp,
    const acc_t* __restrict__ alpha, const acc_t* __restrict__ beta, const acc_t* __restrict__ ll, const int* __restrict__ link,
    const float* __restrict__ grad_out, int grad_out_stride, float scale, float* grad, long ldg) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * CTC_ROW_WAVES + (threadIdx.x >> 6);
    if (row >= (long)B * T) return;
    const int t = (int)(row % T);
    const int b = (int)(row / T);
    const int Tb = clampi(act_lens[b], 1, T), Ub = clampi(label_lens[b], 0, U);
    const acc_t L = ll[b];
    const bool live = (t < Tb) && (L > CTC_DEAD);      // frames past the utterance and utterances without a feasible alignment: zero rows
    const float* r = logits + row * ldv;
    float* g = grad + row * ldg;
    float l = 0.f, gs = 0.f;
    if (live) {
        l = lse[row];
        gs = scale * grad_out[(long)b * grad_out_stride];
    }
    // g * softmax over the whole row; the pad columns are zeroed: the head's dgrad / wgrad GEMMs may run over the full pitch
    row_map<float>(r, g, V, ldg, vec_ok, lane, live, [&](float x, int) -> float { return live ? gs * __expf(x - l) : 0.f; });
    if (!live) return;                                          // (wave-uniform)
    // the columns of the row's own symbols: g * (softmax - sum over the states of that symbol of exp(alpha + beta - lp - ll)).  The wave's
    // softmax stores above are complete before these overwrite them; each column has ONE owner lane that adds its states in label order.
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    const long Sp = ctc_sp(U);
    const double2* a2 = reinterpret_cast<const double2*>(alpha + row * Sp);
    const double2* b2 = reinterpret_cast<const double2*>(beta + row * Sp);
    const float2* e2 = reinterpret_cast<const float2*>(lp + row * Sp);
    const int* lk = link + (long)b * U;
    const int* lab = labels + (long)b * U;
    auto occ = [&](acc_t a, acc_t bt, float e) -> float { return __expf((float)(a + bt - L - (acc_t)e)); };
    float accb = 0.f;
    for (int k = lane; k <= Ub; k += 64) {
        const double2 a = a2[k], be = b2[k];
        const float2 e = e2[k];
        accb += occ(a.x, be.x, e.x);
        if (k < Ub) {
            const int w = lk[k];
            const int y = clampi(lab[k], 0, V - 1);
            if (y == blank) {
                accb += occ(a.y, be.y, e.y);
            } else if (w & LINK_FIRST) {
                float sum = occ(a.y, be.y, e.y);
                for (int j = (w & 0xffff) - 1; j >= 0; j = (lk[j] & 0xffff) - 1) sum += occ(a2[j].y, b2[j].y, e2[j].y);
                g[y] = gs * (__expf(e.y) - sum);
            }
        }
    }
    const float tot = wave_sum(accb);
    if (lane == 0) g[blank] = gs * (__expf(e2[0].x) - tot);
}

// ------------------------------------------------------------------ greedy decode
// One workgroup per utterance.  Its waves take the frames' argmax (tokens[b, t] holds frame t's symbol for a moment), then wave 0 compacts
// the row in place, 64 frames at a time: keep frame t iff its symbol is not blank and differs from frame t-1's.  A kept frame lands at an
// index <= t, and only a frame's own value is ever written at its own index, so the symbols still to be read are intact.
// A frame without a finite maximum (NaN, +inf, or all -inf) gets the symbol the greedy scans give it (rowops.h) and is reported through
// count[b] = -(1 + first such frame).
__global__ __launch_bounds__(256) void ctc_greedy_kernel(const float* __restrict__ logits, long ld, const int* __restrict__ act_lens, int T,
                                                         int V, int blank, int* __restrict__ tokens, int* __restrict__ count) {
    __shared__ int bad;
    const int b = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int Tb = clampi(act_lens[b], 1, T);
    int* tok = tokens + (long)b * T;
    if (threadIdx.x == 0) bad = 0x7fffffff;
    __syncthreads();
    for (int t = wave; t < Tb; t += 4) {
        const float* r = logits + ((long)b * T + t) * ld;
        const int bi = wave_row_argmax(r, V, lane);
        if (lane == 0) {
            tok[t] = bi;
            const float x = r[bi];
            if (!(fabsf(x) < INFINITY)) atomicMin(&bad, t);
        }
    }
    __syncthreads();
    if (wave != 0) return;
    int n = 0, last = -1;                               // tokens kept so far; symbol of the frame before this chunk
    for (int base = 0; base < Tb; base += 64) {
        const int t = base + lane;
        const int a = t < Tb ? tok[t] : blank;
        int prev = __shfl_up(a, 1, 64);
        if (lane == 0) prev = last;
        const bool keep = t < Tb && a != blank && a != prev;
        const unsigned long long mask = __ballot(keep);
        __builtin_amdgcn_wave_barrier();                // every lane has read its frame before any lane writes
        if (keep) tok[n + __popcll(mask & ((1ull << lane) - 1ull))] = a;
        n += __popcll(mask);
        last = __shfl(a, 63, 64);
    }
    if (lane == 0) count[b] = bad != 0x7fffffff ? -(1 + bad) : n;
}

// ------------------------------------------------------------------ forced alignment: best path through the CTC lattice
// v(0,0) = lp(0,0), v(0,1) = lp(0,1), v(t,s) = lp(t,s) + max(v(t-1,s), v(t-1,s-1), v(t-1,s-2)), the s-2 term under the skip rule of the loss.
// It is the alpha half of ctc_alphabeta_kernel with max in place of lae, in the same shape: one workgroup per utterance, thread k owns the
// state pair (2k, 2k+1), "label k-1" arrives by the one-lane DPP rotate, the cell that crosses a wave boundary goes through the
// double-buffered LDS slot (U + 1 <= 64: one wave, no barrier in the walk), emission rows prefetched CTC_PF frames ahead, frontier in fp64.
// TIE RULE: predecessors are tried in the order s, s-1, s-2 and a later one replaces an earlier one only when STRICTLY greater.
// The decision of a blank state is one bit (1 = came from s-1), of a label state two (01 = s-1, 10 = s-2): three __ballot words per frame
// and wave, 1.5 bits per cell, stored by lane 0 at dec[(t * W + wave) * 3 ...] - in LDS when the utterance's words fit, else in the caller's
// workspace.  The backtrace follows in the same kernel on wave 0, serial per utterance: the path ends in S-1 unless v(T_b-1, S-2) is strictly
// greater and steps one frame down per decision; the wave fetches the words of 64 frames at a time (lane j: frame t - j, the wave that owns
// state s) and walks them by lane reads with t and s in scalar registers - a new fetch only after 64 steps or when s leaves that wave's
// states.  s never grows and is clamped at 0, so whatever the workspace holds (NaN included) no index leaves its array.
typedef unsigned long long cdec_t;
constexpr int CTC_DW = 3;                 // decision words per (frame, wave): blank bit, label low bit, label high bit

template <bool MULTI, bool LDS_DEC>
__global__ __launch_bounds__(MULTI ? 1024 : 64) void ctc_viterbi_kernel(
    const float* __restrict__ lp, const int* __restrict__ labels, const int* __restrict__ act_lens, const int* __restrict__ label_lens,
    int T, int U, int V, int blank, cdec_t* __restrict__ dec_ws, int* __restrict__ path, int* __restrict__ spans,
    float* __restrict__ score, int backtrace) {
    extern __shared__ __attribute__((aligned(16))) char ctc_vit_smem[];
    __shared__ acc_t bnd[2][16];          // the label cell that crosses a wave boundary, double-buffered by frame parity
    __shared__ acc_t fin[2];
    const int b = blockIdx.x;
    const int k = threadIdx.x, lane = k & 63, wave = k >> 6, W = blockDim.x >> 6;
    const int Tb = clampi(act_lens[b], 1, T), Ub = clampi(label_lens[b], 0, U);
    const bool vb = k <= Ub, vl = k < Ub;             // this thread's blank / label state exists
    const int* lab = labels + (long)b * U;
    const int yk = vl ? clampi(lab[k], 0, V - 1) : -1;
    const long rp = ctc_sp(U) / 2;                    // pairs per frame
    const int kc = k <= U ? k : U;                    // in-range pair for the (unconditional) loads of the threads that pad the last wave
    const float2* e2 = reinterpret_cast<const float2*>(lp + (long)b * T * ctc_sp(U)) + kc;
    cdec_t* dec_l = reinterpret_cast<cdec_t*>(ctc_vit_smem);                // [T_b][W][3] (LDS_DEC)
    cdec_t* dec_g = dec_ws + (long)b * T * W * CTC_DW;                      // [T][W][3] per utterance (otherwise)
    // skip transition into label state 2k+1 from 2k-1: l'_s != blank and l'_s != l'_{s-2}
    const bool skip = vl && k > 0 && yk != blank && yk != clampi(lab[k > 0 ? k - 1 : 0], 0, V - 1);
    float2 cur[CTC_PF], nxt[CTC_PF];
    const float2 e0 = e2[0];
    acc_t ab = k == 0 ? (acc_t)e0.x : (acc_t)NEG;
    acc_t al = (k == 0 && vl) ? (acc_t)e0.y : (acc_t)NEG;
#pragma unroll
    for (int i = 0; i < CTC_PF; ++i) cur[i] = e2[(long)min(1 + i, Tb - 1) * rp];
    for (int base = 1; base < Tb; base += CTC_PF) {
#pragma unroll
        for (int i = 0; i < CTC_PF; ++i) nxt[i] = e2[(long)min(base + CTC_PF + i, Tb - 1) * rp];
#pragma unroll
        for (int i = 0; i < CTC_PF; ++i) {
            const int t = base + i;
            if (t < Tb) {                              // workgroup-uniform
                if (MULTI) {
                    if (lane == 63) bnd[t & 1][wave] = al;
                    __syncthreads();
                }
                acc_t nb = rot_r1(al);                 // label state of thread k-1 at frame t-1
                if (lane == 0) nb = (MULTI && wave > 0) ? bnd[t & 1][wave > 0 ? wave - 1 : 0] : (acc_t)NEG;
                const bool db = vb && k > 0 && nb > ab;                    // blank state: s, then s-1
                const acc_t nab = vb ? (acc_t)cur[i].x + (db ? nb : ab) : (acc_t)NEG;
                acc_t m = al;                                              // label state: s, then s-1, then s-2
                const bool d1 = vl && ab > m;
                m = d1 ? ab : m;
                const bool d2 = skip && nb > m;
                m = d2 ? nb : m;
                al = vl ? (acc_t)cur[i].y + m : (acc_t)NEG;
                ab = nab;
                const cdec_t w0 = __ballot(db), w1 = __ballot(d1 && !d2), w2 = __ballot(d2);
                if (lane == 0) {
                    const long o = ((long)t * W + wave) * CTC_DW;
                    if constexpr (LDS_DEC) { dec_l[o] = w0; dec_l[o + 1] = w1; dec_l[o + 2] = w2; }
                    else { dec_g[o] = w0; dec_g[o + 1] = w1; dec_g[o + 2] = w2; }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < CTC_PF; ++i) cur[i] = nxt[i];
    }
    // the path ends in S-1 = 2 U_b (thread U_b's blank) unless S-2 (thread U_b - 1's label) is strictly greater
    if (k == Ub) fin[0] = ab;
    if (Ub > 0 && k == Ub - 1) fin[1] = al;
    if constexpr (!LDS_DEC) __threadfence();
    __syncthreads();                                   // ... and lane 0's decision words are visible to wave 0
    const acc_t endb = fin[0], endl = Ub > 0 ? fin[1] : (acc_t)NEG;
    const bool end_lab = Ub > 0 && endl > endb;
    const acc_t best = end_lab ? endl : endb;
    const bool dead = best <= CTC_DEAD;                // no feasible alignment, by the loss's threshold (a NaN stays a NaN)
    int* pr = path + (long)b * T;
    int* sp = spans + (long)b * U * 2;
    for (int t = (dead ? 0 : Tb) + k; t < T; t += blockDim.x) pr[t] = -1;
    for (int i = (dead ? 0 : 2 * Ub) + k; i < 2 * U; i += blockDim.x) sp[i] = -1;
    if (k == 0) score[b] = dead ? -INFINITY : (float)best;
    if (dead || !backtrace || wave != 0) return;       // (ttmi_set_option(23, 2): the forward walk alone, measurement only)
    int t = Tb - 1, s = end_lab ? 2 * Ub - 1 : 2 * Ub;
    int last = t;                                      // last frame of the run of states the walk is in
    while (t >= 0) {
        const int g = s >> 7;                          // the wave that owns state s
        const int tl = t - lane;
        cdec_t w[CTC_DW] = {0, 0, 0};
        if (tl >= 1) {                                 // frame 0 has no predecessor and no words
            const long o = ((long)tl * W + g) * CTC_DW;
#pragma unroll
            for (int i = 0; i < CTC_DW; ++i) {
                if constexpr (LDS_DEC) w[i] = dec_l[o + i];
                else w[i] = dec_g[o + i];
            }
        }
        int lo[CTC_DW], hi[CTC_DW];
#pragma unroll
        for (int i = 0; i < CTC_DW; ++i) {
            lo[i] = (int)(unsigned)(w[i] & 0xffffffffULL);
            hi[i] = (int)(unsigned)(w[i] >> 32);
        }
        const int t0 = t;
        int mine = -1, j = 0;
        for (; j < 64 && t >= 0 && (s >> 7) == g; ++j, --t) {
            mine = lane == j ? s : mine;
            const int q = (s >> 1) & 63;
            auto bit = [&](int i) -> int {
                const unsigned x = (unsigned)((q & 32) ? __builtin_amdgcn_readlane(hi[i], j) : __builtin_amdgcn_readlane(lo[i], j));
                return (int)((x >> (q & 31)) & 1u);
            };
            int d = 0;
            if (t > 0) d = (s & 1) ? bit(1) + 2 * bit(2) : bit(0);
            if (d > s) d = s;
            if (d != 0 || t == 0) {                    // frame t opens the run: a label state's span is (t, last)
                if ((s & 1) && lane == 0) {
                    sp[s - 1] = t;
                    sp[s] = last;
                }
                last = t - 1;
            }
            s -= d;
        }
        if (lane < j) pr[t0 - lane] = mine;
    }
}

// Per label, from a finished forward: the occupancy g(t,s) = exp(alpha(t,s) + beta(t,s) - lp(t,s) - ll) of its state s = 2u+1 and the
// posterior e(t,u) that its run starts at frame t - e(t,u) = exp(logsumexp(alpha(t-1,s-1), alpha(t-1,s-2) [skip rule]) + beta(t,s) - ll) for
// t > 0 (beta includes the emission at t), e(0,0) = g(0,1), e(0,u>0) = 0.  mass = sum_t e (every alignment enters every label state exactly
// once: 1, a health check of the lattice), expected = sum_t t e, duration = sum_t g.  One workgroup per (utterance, 64 labels), lanes across
// u, so every load of the time-major tables is one row segment.  The TERMS of a chunk of 32 frames are formed by all eight waves (four frames
// each, their loads in flight together: the kernel is bound by load latency) and handed over in LDS as the f32 values the exponential
// returns; the SUMS have one owner, lane u of wave 0, which adds the chunk's terms in frame order in fp64 - the order of a serial loop over
// t, whatever the wave count.  The hand-over is double-buffered by chunk parity: one barrier per chunk.  No atomics.  Entries u >= U_b and
// utterances without a feasible alignment: mass 0, expected -1, duration 0.
constexpr int CTC_ES_WAVES = 8, CTC_ES_F = 4, CTC_ES_CHUNK = CTC_ES_WAVES * CTC_ES_F;

__global__ __launch_bounds__(CTC_ES_WAVES * 64) void ctc_emit_stats_kernel(
    const acc_t* __restrict__ alpha, const acc_t* __restrict__ beta, const acc_t* __restrict__ ll, const float* __restrict__ lp,
    const int* __restrict__ labels, const int* __restrict__ act_lens, const int* __restrict__ label_lens, int T, int U, int V, int blank,
    int G, float* __restrict__ expected, float* __restrict__ mass, float* __restrict__ duration) {
    __shared__ float2 part[2][CTC_ES_CHUNK][64];       // (e, g) of a chunk's frames
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int b = blockIdx.x / G;
    const int u = (blockIdx.x % G) * 64 + lane;
    const int Tb = clampi(act_lens[b], 1, T), Ub = clampi(label_lens[b], 0, U);
    const acc_t L = ll[b];
    const bool live = L > CTC_DEAD;                    // workgroup-uniform
    const bool has = live && u < Ub;
    acc_t m = 0.0, e1 = 0.0, dur = 0.0;
    if (live) {
        const int uc = has ? u : 0;                    // lanes without a label form in-range addresses and load nothing
        const int* lab = labels + (long)b * U;
        const int yu = has ? clampi(lab[uc], 0, V - 1) : -1;
        const bool skip = has && u > 0 && yu != blank && yu != clampi(lab[uc > 0 ? uc - 1 : 0], 0, V - 1);
        const long rp = ctc_sp(U) / 2;
        const double2* a2 = reinterpret_cast<const double2*>(alpha + (long)b * T * ctc_sp(U)) + uc;
        const double2* b2 = reinterpret_cast<const double2*>(beta + (long)b * T * ctc_sp(U)) + uc;
        const float2* e2 = reinterpret_cast<const float2*>(lp + (long)b * T * ctc_sp(U)) + uc;
        for (int base = 0, c = 0; base < Tb; base += CTC_ES_CHUNK, ++c) {
            float2 v[CTC_ES_F];
#pragma unroll
            for (int i = 0; i < CTC_ES_F; ++i) {
                const int t = base + wv * CTC_ES_F + i;
                v[i] = make_float2(0.f, 0.f);
                if (has && t < Tb) {
                    const long o = (long)t * rp;
                    const acc_t bt = b2[o].y;
                    const float g = __expf((float)(a2[o].y + bt - (acc_t)e2[o].y - L));
                    float e = u == 0 ? g : 0.f;        // frame 0: e(0,0) = g(0,1), e(0,u>0) = 0
                    if (t > 0) {
                        acc_t in = a2[o - rp].x;       // alpha(t-1, 2u)
                        if (skip) in = lae(in, a2[o - rp - 1].y);      // alpha(t-1, 2u-1): the label state of pair u-1
                        e = __expf((float)(in + bt - L));
                    }
                    v[i] = make_float2(e, g);
                }
            }
#pragma unroll
            for (int i = 0; i < CTC_ES_F; ++i) part[c & 1][wv * CTC_ES_F + i][lane] = v[i];
            __syncthreads();
            if (wv == 0) {
                const int n = min(CTC_ES_CHUNK, Tb - base);
                for (int f = 0; f < n; ++f) {
                    const float2 x = part[c & 1][f][lane];
                    m += (acc_t)x.x;
                    e1 += (acc_t)(base + f) * (acc_t)x.x;
                    dur += (acc_t)x.y;
                }
            }
        }
    }
    if (wv == 0 && u < U) {
        const long i = (long)b * U + u;
        mass[i] = has ? (float)m : 0.f;
        expected[i] = has ? (float)e1 : -1.f;
        duration[i] = has ? (float)dur : 0.f;
    }
}

__host__ __forceinline__ size_t ctc_dec_bytes(int T, int U) { return (size_t)T * ((U + 1 + 63) / 64) * CTC_DW * sizeof(cdec_t); }

}  // namespace

int ttmi_rnnt_get_align_debug();          // rnnt.hip: ttmi_set_option(23, bits), shared with ttmi_rnnt_align / ttmi_mono_align

extern "C" {

// Forced alignment and emission statistics from the workspace a finished ttmi_ctc_loss_fwd left on the same (B, T, U); that workspace is
// only read (include/ttmi.h).  No host synchronisation, no memset node: both are capturable in a HIP graph.
size_t ttmi_ctc_align_workspace_bytes(int B, int T, int U) {
    if (B <= 0 || T <= 0 || U < 0 || U > 1023) return 0;
    return (size_t)B * ctc_dec_bytes(T, U);
}

int ttmi_ctc_align(const void* workspace, const int* labels, const int* act_lens, const int* label_lens, int B, int T, int U, int V, int blank,
                   void* align_workspace, int* path, int* spans, float* score, void* stream) {
    TTMI_REQUIRE(workspace && (labels || U == 0) && act_lens && label_lens && align_workspace && path && (spans || U == 0) && score,
                 "ctc_align: null pointer");
    TTMI_REQUIRE(B > 0 && T > 0 && U >= 0 && V >= 2, "ctc_align: bad shape B=%d T=%d U=%d V=%d", B, T, U, V);
    TTMI_REQUIRE(U <= 1023, "ctc_align: U=%d > 1023 unsupported", U);
    TTMI_REQUIRE(blank >= 0 && blank < V, "ctc_align: blank %d outside [0,%d)", blank, V);
    TTMI_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "ctc_align: workspace must be 16-byte aligned");
    TTMI_REQUIRE((reinterpret_cast<uintptr_t>(align_workspace) & 7) == 0, "ctc_align: align_workspace must be 8-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const CtcWs w = ctc_carve(const_cast<void*>(workspace), B, T, U);
    cdec_t* dec = static_cast<cdec_t*>(align_workspace);
    const int debug = ttmi_rnnt_get_align_debug();
    const int threads = cdiv(U + 1, 64) * 64;
    auto launch = [&](auto k_lds, auto k_ws) {
        return launch_dec_lds("ctc align", k_lds, k_ws, ctc_dec_bytes(T, U), debug, dim3(B), dim3(threads), st, w.lp, labels, act_lens, label_lens, T,
                              U, V, blank, dec, path, spans, score);
    };
    const int rc = threads == 64 ? launch(ctc_viterbi_kernel<false, true>, ctc_viterbi_kernel<false, false>)
                                 : launch(ctc_viterbi_kernel<true, true>, ctc_viterbi_kernel<true, false>);
    if (rc) return rc;
    TTMI_LAUNCH_CHECK("ctc_viterbi_kernel");
    return TTMI_OK;
}

int ttmi_ctc_emit_stats(const void* workspace, const int* labels, const int* act_lens, const int* label_lens, int B, int T, int U, int V,
                        int blank, float* expected, float* mass, float* duration, void* stream) {
    TTMI_REQUIRE(workspace && act_lens && label_lens && ((labels && expected && mass && duration) || U == 0), "ctc_emit_stats: null pointer");
    TTMI_REQUIRE(B > 0 && T > 0 && U >= 0 && V >= 2, "ctc_emit_stats: bad shape B=%d T=%d U=%d V=%d", B, T, U, V);
    TTMI_REQUIRE(U <= 1023, "ctc_emit_stats: U=%d > 1023 unsupported", U);
    TTMI_REQUIRE(blank >= 0 && blank < V, "ctc_emit_stats: blank %d outside [0,%d)", blank, V);
    TTMI_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "ctc_emit_stats: workspace must be 16-byte aligned");
    if (U == 0) return TTMI_OK;           // no labels: nothing to write
    const CtcWs w = ctc_carve(const_cast<void*>(workspace), B, T, U);
    const int G = cdiv(U, 64);
    hipLaunchKernelGGL(ctc_emit_stats_kernel, dim3((unsigned)((long)B * G)), dim3(CTC_ES_WAVES * 64), 0, static_cast<hipStream_t>(stream), w.alpha, w.beta, w.ll,
                       w.lp, labels, act_lens, label_lens, T, U, V, blank, G, expected, mass, duration);
    TTMI_LAUNCH_CHECK("ctc_emit_stats_kernel");
    return TTMI_OK;
}

// bytes of caller-provided workspace shared by ttmi_ctc_loss_fwd / _bwd (16-byte aligned): lp table, alpha, beta, ll, lse, symbol chains
size_t ttmi_ctc_workspace_bytes(int B, int T, int U) {
    if (B <= 0 || T <= 0 || U < 0) return 0;
    const size_t n = (size_t)B * T * ctc_sp(U);
    return sizeof(acc_t) * (2 * n + even(B)) + sizeof(float) * (even((long)B * T) + n) + sizeof(int) * ((size_t)B * (U > 0 ? U : 1)) + 64;
}

int ttmi_ctc_loss_fwd(const float* logits, long ldv, const int* labels, const int* act_lens, const int* label_lens, int B, int T, int U,
                      int V, int blank, void* workspace, float* costs, void* stream) {
    TTMI_REQUIRE(logits && (labels || U == 0) && act_lens && label_lens && workspace && costs, "ctc_loss_fwd: null pointer");
    TTMI_REQUIRE(B > 0 && T > 0 && U >= 0 && V > 0, "ctc_loss_fwd: bad shape B=%d T=%d U=%d V=%d", B, T, U, V);
    TTMI_REQUIRE(ldv >= V, "ctc_loss_fwd: bad pitch");
    TTMI_REQUIRE(blank >= 0 && blank < V, "ctc_loss_fwd: blank %d outside [0,%d)", blank, V);
    TTMI_REQUIRE(U <= 1023, "ctc_loss_fwd: U=%d > 1023 unsupported", U);
    TTMI_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "ctc_loss_fwd: workspace must be 16-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    CtcWs w = ctc_carve(workspace, B, T, U);
    const long rows = (long)B * T;
    const int vec_ok = rows_vec_ok(logits, 4);
    if (U > 0) {
        hipLaunchKernelGGL(ctc_link_kernel, dim3(B), dim3(256), 0, st, labels, label_lens, U, V, blank, w.link);
        TTMI_LAUNCH_CHECK("ctc_link_kernel");
    }
    hipLaunchKernelGGL(ctc_lse_kernel<true>, dim3(cdiv(rows, CTC_ROW_WAVES)), dim3(CTC_ROW_WAVES * 64), 0, st, logits, ldv, labels, act_lens,
                       label_lens, B, T, U, V, blank, vec_ok, w.lse, w.lp);
    TTMI_LAUNCH_CHECK("ctc_lse_kernel");
    const int threads = cdiv(U + 1, 64) * 64;
    if (threads == 64)
        hipLaunchKernelGGL(ctc_alphabeta_kernel<false>, dim3(2 * B), dim3(64), 0, st, w.lp, labels, act_lens, label_lens, T, U, V, blank,
                           w.alpha, w.beta, w.ll, costs);
    else
        hipLaunchKernelGGL(ctc_alphabeta_kernel<true>, dim3(2 * B), dim3(threads), 0, st, w.lp, labels, act_lens, label_lens, T, U, V, blank,
                           w.alpha, w.beta, w.ll, costs);
    TTMI_LAUNCH_CHECK("ctc_alphabeta_kernel");
    return TTMI_OK;
}

int ttmi_ctc_loss_bwd(const float* logits, long ldv, const int* labels, const int* act_lens, const int* label_lens, int B, int T, int U,
                      int V, int blank, const void* workspace, const float* grad_out, int grad_out_stride, float scale, float* grad,
                      long ldg, void* stream) {
    TTMI_REQUIRE(logits && (labels || U == 0) && act_lens && label_lens && workspace && grad_out && grad, "ctc_loss_bwd: null pointer");
    TTMI_REQUIRE(B > 0 && T > 0 && U >= 0 && V > 0, "ctc_loss_bwd: bad shape B=%d T=%d U=%d V=%d", B, T, U, V);
    TTMI_REQUIRE(ldv >= V && ldg >= V, "ctc_loss_bwd: bad pitch");
    TTMI_REQUIRE(blank >= 0 && blank < V, "ctc_loss_bwd: blank %d outside [0,%d)", blank, V);
    TTMI_REQUIRE(U <= 1023, "ctc_loss_bwd: U=%d > 1023 unsupported", U);
    TTMI_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "ctc_loss_bwd: workspace must be 16-byte aligned");
    TTMI_REQUIRE(static_cast<const void*>(logits) != static_cast<const void*>(grad) || ldg == ldv, "ctc_loss_bwd: in-place needs ldg == ldv");
    hipStream_t st = static_cast<hipStream_t>(stream);
    CtcWs w = ctc_carve(const_cast<void*>(workspace), B, T, U);
    const long rows = (long)B * T;
    const int vec_ok = rows_vec_ok(logits, grad, ldv, ldg, 4);
    hipLaunchKernelGGL(ctc_grad_kernel, dim3(cdiv(rows, CTC_ROW_WAVES)), dim3(CTC_ROW_WAVES * 64), 0, st, logits, ldv, labels, act_lens,
                       label_lens, B, T, U, V, blank, vec_ok, w.lse, w.lp, w.alpha, w.beta, w.ll, w.link, grad_out, grad_out_stride, scale,
                       grad, ldg);
    TTMI_LAUNCH_CHECK("ctc_grad_kernel");
    return TTMI_OK;
}

// Full-sum CTC log-likelihood of P hypotheses on the logits of their utterances (include/ttmi.h): the log-sum-exp of every row once per
// utterance into `workspace`, then one workgroup per pair.  No allocation, host synchronisation, memset node or atomics.
size_t ttmi_ctc_score_ws_bytes(int B, int T) {
    if (B <= 0 || T <= 0) return 0;
    return (sizeof(float) * (size_t)B * T + 15) & ~(size_t)15;
}

int ttmi_ctc_score_hyps(const float* logits, long ldv, const int* act_lens, int B, int T, int V, int blank, const long* hyp, long ld_hyp,
                        const int* hyp_len, const int* utt, int P, int U, void* workspace, double* score, void* stream) {
    TTMI_REQUIRE(logits && act_lens && (hyp || U == 0) && hyp_len && workspace && score, "ctc_score_hyps: null pointer");
    TTMI_REQUIRE(B > 0 && T > 0 && P > 0 && V >= 2, "ctc_score_hyps: bad shape B=%d T=%d P=%d V=%d", B, T, P, V);
    TTMI_REQUIRE(U >= 0, "ctc_score_hyps: bad shape U=%d", U);
    TTMI_REQUIRE(U <= 1023, "ctc_score_hyps: U=%d > 1023 unsupported", U);
    TTMI_REQUIRE(U <= ld_hyp, "ctc_score_hyps: U=%d above the hypothesis pitch %ld", U, ld_hyp);
    TTMI_REQUIRE(ldv >= V, "ctc_score_hyps: bad pitch");
    TTMI_REQUIRE(blank >= 0 && blank < V, "ctc_score_hyps: blank %d outside [0,%d)", blank, V);
    TTMI_REQUIRE(utt || P % B == 0, "ctc_score_hyps: without utt P=%d must be a multiple of B=%d", P, B);
    TTMI_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "ctc_score_hyps: workspace must be 16-byte aligned");
    TTMI_REQUIRE((reinterpret_cast<uintptr_t>(score) & 7) == 0, "ctc_score_hyps: score must be 8-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    float* lse = static_cast<float*>(workspace);
    const long rows = (long)B * T;
    hipLaunchKernelGGL(ctc_lse_kernel<false>, dim3(cdiv(rows, CTC_ROW_WAVES)), dim3(CTC_ROW_WAVES * 64), 0, st, logits, ldv,
                       static_cast<const int*>(nullptr), act_lens, static_cast<const int*>(nullptr), B, T, 0, V, blank, rows_vec_ok(logits, 4), lse,
                       static_cast<float*>(nullptr));
    TTMI_LAUNCH_CHECK("ctc_lse_kernel");
    const int threads = cdiv(U + 1, 64) * 64;
    const int per = utt ? 1 : P / B;
    if (threads == 64)
        hipLaunchKernelGGL(ctc_score_kernel<false>, dim3(P), dim3(64), 0, st, logits, ldv, lse, act_lens, B, T, V, blank, hyp, ld_hyp, hyp_len,
                           utt, per, U, score);
    else
        hipLaunchKernelGGL(ctc_score_kernel<true>, dim3(P), dim3(threads), 0, st, logits, ldv, lse, act_lens, B, T, V, blank, hyp, ld_hyp,
                           hyp_len, utt, per, U, score);
    TTMI_LAUNCH_CHECK("ctc_score_kernel");
    return TTMI_OK;
}

int ttmi_ctc_greedy(const float* logits, long ld, const int* act_lens, int B, int T, int V, int blank, int* tokens, int* count,
                    void* stream) {
    TTMI_REQUIRE(logits && act_lens && tokens && count, "ctc_greedy: null pointer");
    TTMI_REQUIRE(B > 0 && T > 0 && V > 0 && ld >= V, "ctc_greedy: bad shape B=%d T=%d V=%d ld=%ld", B, T, V, ld);
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(ctc_greedy_kernel, dim3(B), dim3(256), 0, st, logits, ld, act_lens, T, V, blank, tokens, count);
    TTMI_LAUNCH_CHECK("ctc_greedy_kernel");
    return TTMI_OK;
}

}  // extern "C"
