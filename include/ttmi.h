/* libttmi - MI355X-native Transformer-Transducer hot path, C ABI.
 *
 * Every entry point: plain pointers and sizes, no torch types; all pointers are
 * DEVICE pointers unless noted; `stream` is a hipStream_t (0 = default stream);
 * nothing is allocated or freed inside (ctx / workspace arenas are caller-provided,
 * sizes via the *_floats / *_bytes queries, 256-byte aligned); launches are
 * asynchronous on `stream`, no device-wide sync.
 * Return value: 0 ok, <0 invalid argument (message in ttmi_last_error()), >0 a
 * hipError_t.  No C++ exception crosses the boundary.
 *
 * The reference (zzpDapeng/Transformer-Transducer) is pure Python and has no FFI
 * layer; each function cites the reference lines whose arithmetic it replaces
 * (paths relative to the reference root).  The Python classes that bind these are
 * in transformer-transducer_amd/{tt,warprnnt_pytorch}; see INTEGRATION.md.
 *
 * Conventions
 *   prec        0 = exact-f32 MFMA (v_mfma_f32_32x32x2_f32), all activations f32:
 *                   the parity path (loss/grads within 1e-4 rel of the reference).
 *               1 = bf16 MFMA, f32 accumulate; activations that feed GEMMs are bf16
 *                   in HBM (q/k/v, attention output, FFN inner, joint hidden, logits),
 *                   residual stream / LayerNorm / softmax / lattice stay f32(/f64).
 *   dropout     p_drop / p_layer = drop probabilities (0 in eval).  Masks are counter-based: element i of site s is kept
 *               iff hash(seed ^ salt_s, i) >= p * 2^32 and scaled by 1/(1-p); backward regenerates them from the same
 *               seed.  Sites (reference modules): attention `drop` (tt/transformer.py:173) salt 0xA1, FFN CoreNet.2 /
 *               CoreNet.4 (:47,49) salts 0xB2 / 0xC3, RelLearnableDecoderLayer.dropout (:196) salt 0xD4 (p_layer,
 *               fused into the FFN's output LayerNorm).  ttmi_dropout_apply exposes the same masks.
 *   g_*         parameter-gradient buffers are ACCUMULATED into (+=): zero them once
 *               per optimiser step (optimizer.zero_grad()).
 *   batch-major activations are [B, L, d] row-major (the reference's [L, B, d] layout is
 *               only a transpose away and no op mixes batch elements).
 */
#ifndef TTMI_H
#define TTMI_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

int ttmi_version(void);
const char* ttmi_last_error(void);   /* thread-local, valid until the next failing call */

/* ---- relative-position self-attention sub-layer ------------------------------------------------------
 * RelLearnableMultiHeadAttn.forward incl. _rel_shift, mask, softmax, o_net, residual + LayerNorm
 * (tt/transformer.py:82-89,106-177).  x,y f32 [B,L,d]; qkv_w [3*H*Dh, d]; o_w [d, H*Dh]; r_emb [K,H,Dh];
 * r_w_bias [H,Dh]; r_bias [K,H].  mask_kind 0 none | 1 causal (tt/utils.py:233-239) | 2 band: masked iff
 * j > i+right or j < i-left (tt/utils.py:242-251) | 3 uint8 tensor, element (b,i,j) at
 * mask[b*mask_sb + i*mask_si + j], nonzero = masked (any [L,L,1] / [L,L,B] / (klen,bsz) mask of
 * tt/transformer.py:154-159 after a permute) | 4 per-row key intervals: `mask` points at int32 pairs, (lo, hi) of query i of batch b at
 * ((const int*)mask)[b*mask_sb + 2*i], key j masked iff j < lo or j > hi (what chunk / band masks are; mask_sb = 0 shares one table);
 * with kind 4, mask_left / mask_right may carry bounds on the intervals' reach from the diagonal (lo_i >= i - left, hi_i <= i + right,
 * -1 / -1 or 0 / 0 = not known).  The fused attention kernels skip key tiles that are masked for a whole query block (kinds 1, 2, 4),
 * and for narrow bands (kind 2, or kind 4 with bounds) the backward also skips the query tiles a key block never meets. */
size_t ttmi_attn_ctx_floats(int B, int L, int d, int H, int Dh, int prec);
size_t ttmi_attn_ws_floats(int B, int L, int d, int H, int Dh, int prec);
int ttmi_attn_fwd(const float* x, const float* qkv_w, const float* o_w, const float* ln_g, const float* ln_b,
                  const float* r_emb, const float* r_w_bias, const float* r_bias, int B, int L, int d, int H, int Dh, int K,
                  int mask_kind, int mask_left, int mask_right, const unsigned char* mask, long mask_sb, long mask_si,
                  int prec, float p_drop, unsigned seed, float* ctx, float* ws, float* y, void* stream);
int ttmi_attn_bwd(const float* dy, const float* x, const float* qkv_w, const float* o_w, const float* ln_g,
                  const float* r_emb, const float* r_w_bias, const float* r_bias, int B, int L, int d, int H, int Dh, int K, int mask_kind,
                  int mask_left, int mask_right, const unsigned char* mask, long mask_sb, long mask_si, int prec,
                  float p_drop, unsigned seed, const float* ctx, float* ws, float* dx, float* g_qkv_w, float* g_o_w,
                  float* g_ln_g, float* g_ln_b, float* g_r_emb, float* g_r_w_bias, float* g_r_bias, void* stream);

/* ---- position-wise feed-forward sub-layer -----------------------------------------------------------------
 * PositionwiseFF.forward: z = LN(y + W2 relu(W1 LN(y) + b1) + b2), ONE LayerNorm used twice
 * (tt/transformer.py:36-58).  rows = B*L; w1 [Di,d]; w2 [d,Di]. */
size_t ttmi_ffn_ctx_floats(long rows, int d, int Di, int prec);
size_t ttmi_ffn_ws_floats(long rows, int d, int Di, int prec);
int ttmi_ffn_fwd(const float* y, const float* w1, const float* b1, const float* w2, const float* b2, const float* ln_g,
                 const float* ln_b, long rows, int d, int Di, int prec, float p_drop, float p_layer, unsigned seed, float* ctx,
                 float* ws, float* z, void* stream);
int ttmi_ffn_bwd(const float* dz, const float* y, const float* w1, const float* w2, const float* ln_g, long rows, int d, int Di,
                 int prec, float p_drop, float p_layer, unsigned seed, const float* ctx, float* ws, float* dy, float* g_w1,
                 float* g_b1, float* g_w2, float* g_b2, float* g_ln_g, float* g_ln_b, void* stream);

/* ---- label-encoder embedding: nn.Embedding(V, d, padding_idx=0) (tt/decoder.py:26,39) ------------------------ */
int ttmi_embed_fwd(const long* tokens, const float* W, long n, int d, int V, float* out, void* stream);
int ttmi_embed_bwd(const long* tokens, const float* dout, long n, int d, int V, int padding_idx, float* gW, void* stream);

/* ---- joint network: JointNet.forward (tt/model.py:20-39) in split-weight form ---------------------------------
 * logits[b,t,u,:] = wp tanh(wf[:, :de] enc[b,t] + wf[:, de:] dec[b,u] + bf) + bp.  enc [B,T,de], dec [B,U1,dd],
 * wf [J, de+dd], wp [V,J].  ttmi_joint_logits_dtype(prec,J): 0 -> logits/dlogits are f32, 1 -> bf16.  Rows
 * (b,t,u) of logits/dlogits have pitch ldv/ldg >= V elements; in the bf16 case the pitch must be a multiple of 8,
 * the base 16-byte aligned, and dlogits must be ZERO in columns [V, ldg) (ttmi_rnnt_loss_bwd guarantees it). */
int ttmi_joint_logits_dtype(int prec, int J);
size_t ttmi_joint_ctx_floats(int B, int T, int U1, int J);
size_t ttmi_joint_ws_floats(int B, int T, int U1, int J, int V);
/* the same for a given precision code: prec 2 (TTMI_PRECISION=bf16x3: the f32 data flow of prec 0 with its large dense products on the bf16
 * MFMA in three terms, hi . hi + lo . hi + hi . lo) needs room for the split operands behind the ordinary workspace */
size_t ttmi_joint_ws_floats_prec(int B, int T, int U1, int J, int V, int prec);
/* ... and ctx: prec 2 keeps the hidden rows as two bf16 blocks [hi | lo] instead of one f32, columns padded to a multiple of 64: callers that
 * pass prec 2 to ttmi_joint_fwd / ttmi_joint_bwd size ctx with this one (the same size as ttmi_joint_ctx_floats when J % 64 == 0) */
size_t ttmi_joint_ctx_floats_prec(int B, int T, int U1, int J, int prec);
int ttmi_joint_fwd(const float* enc, const float* dec, const float* wf, const float* bf, const float* wp, const float* bp,
                   int B, int T, int U1, int de, int dd, int J, int V, int prec, float* ctx, float* ws, void* logits, long ldv,
                   void* stream);
int ttmi_joint_bwd(const void* dlogits, long ldg, const float* enc, const float* dec, const float* wf, const float* wp, int B,
                   int T, int U1, int de, int dd, int J, int V, int prec, const float* ctx, float* ws, float* denc, float* ddec,
                   float* g_wf, float* g_bf, float* g_wp, float* g_bp, void* stream);

/* ---- RNN-T loss: replaces warprnnt_pytorch.RNNTLoss (train.py:13,53,231) --------------------------------------
 * logits [B,T,U1,V] (dtype 0 = f32, 1 = bf16), row pitch ldv; labels i32 [B,U1-1]; act_lens,label_lens i32 [B];
 * costs f32 [B] = -log P(y|x).  bwd: grad = scale * grad_out[b*grad_out_stride] * d costs[b]/d logits in the logits'
 * dtype with row pitch ldg (columns [V,ldg) zeroed); grad may alias logits when ldg == ldv. */
size_t ttmi_rnnt_workspace_bytes(int B, int T, int U1);
int ttmi_rnnt_loss_fwd(const void* logits, int dtype, long ldv, const int* labels, const int* act_lens, const int* label_lens,
                       int B, int T, int U1, int V, int blank, void* workspace, float* costs, void* stream);
int ttmi_rnnt_loss_bwd(const void* logits, int dtype, long ldv, const int* labels, const int* act_lens, const int* label_lens,
                       int B, int T, int U1, int V, int blank, const void* workspace, const float* grad_out,
                       int grad_out_stride, float scale, void* grad, long ldg, void* stream);
/* bf16x3 mode (TTMI_PRECISION=bf16x3, prec 2; no reference counterpart - the reference's loss is warprnnt_pytorch's, tt/model.py:5): the gradient of f32 logits
 * written OVER them as the two bf16 planes the three-term joint backward multiplies - row r becomes [hi(0 .. ldv) | lo(0 .. ldv)], hi = bf16(g), lo = bf16(g - hi),
 * 2 ldv bf16 in the bytes of ldv f32, columns [V, ldv) zero in both planes - so that ttmi_joint_bwd_split need not read d logits again to split them.  Ask the two
 * _ok functions first (rows 16-byte aligned, pitch == roundup(V, 64), the product large enough for the three-term kernels); otherwise use ttmi_rnnt_loss_bwd +
 * ttmi_joint_bwd.  Workspace / grad_out / scale as in ttmi_rnnt_loss_bwd; the other arguments of ttmi_joint_bwd_split as in ttmi_joint_bwd. */
int ttmi_rnnt_loss_bwd_split_ok(long ldv, const void* logits);
int ttmi_rnnt_loss_bwd_split(void* logits, long ldv, const int* labels, const int* act_lens, const int* label_lens, int B, int T, int U1, int V,
                             int blank, const void* workspace, const float* grad_out, int grad_out_stride, float scale, void* stream);
int ttmi_joint_bwd_split_ok(int B, int T, int U1, int J, int V, int prec, long ldg);
int ttmi_joint_bwd_split(const void* dlogits_split, long ldg, const float* enc, const float* dec, const float* wf, const float* wp, int B,
                         int T, int U1, int de, int dd, int J, int V, int prec, const float* ctx, float* ws, float* denc, float* ddec,
                         float* g_wf, float* g_bf, float* g_wp, float* g_bp, void* stream);

/* ---- fused joint + loss fast path ("exp-domain" forms; training-sized bf16 problems, ask ttmi_joint_exp_supported first) --------
 * Replaces the pair JointNet.forward + RNNTLoss (train.py:47-53) when the caller wants the loss only.  The projection GEMM's epilogue
 * stores P[row, v] = bf16(exp(logit - *shift)) (pitch ldv, a multiple of 64, zeros in columns [V, ldv)) and per-row partial sums of the
 * unrounded values (rowsum f32 [nparts, rows], nparts = ttmi_joint_exp_nparts(V)); the loss forward then reads the sums and two entries
 * per row instead of walking the lattice's rows; the loss backward writes per-row factors srow (f32) / srow16 (bf16) and patches the
 * blank / label entries of P so that d logits[r, :] = srow[r] * P[r, :]; ttmi_joint_bwd_exp consumes that product without forming it
 * (row factor in the dgrad epilogue and on the wgrad's activation operand; ctx is overwritten).
 * shift / shift_cur: device scalar (nullable = 0) subtracted before exp; shift_next (device scalar, nullable):
 * max(itself, max_rows(log-sum-exp) - 40), the value to pass as shift on the next step.
 * emis (nullable, f32 [rows, 4], 16-byte aligned): ttmi_joint_fwd_exp also leaves the logits of `blank` and of each row's next label
 * (labels int32 [B, U1-1]) in f32, twice: formed from the bf16 operands the projection multiplies (entries 0, 1: what P and its row
 * sums contain) and from the unrounded hidden row with the f32 weight (entries 2, 3).  ttmi_rnnt_loss_fwd_exp exchanges the two columns'
 * terms of the row sum for the accurate ones and takes the emission log-probs from entries 2, 3: the bf16 rounding of the projection
 * weight is the same in every row, so the blank column's error does not average out along an alignment.
 * flag (nullable, device int): bit 0 is set when a lattice row's sum underflowed or overflowed (the shift no longer fits the logits);
 * the costs and gradients of that step are then NaN (never finite-and-wrong): drop the step, run one step in the plain form and take a new
 * shift from its workspace with ttmi_rnnt_shift_seed (no host synchronisation anywhere in the protocol). */
int ttmi_joint_exp_supported(int B, int T, int U1, int J, int V, int prec, long ldv);
int ttmi_joint_exp_fwd_supported(int B, int T, int U1, int J, int V, int prec, long ldv);     /* forward + loss only (no gradients wanted) */
int ttmi_joint_exp_nparts(int V);
/* lattice rows of a chunk padded to the exp-domain wgrad's 64-row reduction tile: the row count P / srow / srow16 / emis / ctx must have
 * room for (the pad rows get zero row factors and add exact zeros; tt/model.py:20-39 has no counterpart - the reference materialises
 * [B, T, U+1, V] logits of exactly B*T*U1 rows) */
long ttmi_joint_exp_padded_rows(int B, int T, int U1);
int ttmi_joint_fwd_exp(const float* enc, const float* dec, const float* wf, const float* bf, const float* wp, const float* bp,
                       int B, int T, int U1, int de, int dd, int J, int V, int prec, float* ctx, float* ws, void* P, long ldv,
                       float* rowsum, int nparts, const float* shift, const int* labels, int blank, float* emis, void* stream);
int ttmi_rnnt_loss_fwd_exp(const void* P, long ldv, const float* rowsum, int nparts, const int* labels, const int* act_lens,
                           const int* label_lens, int B, int T, int U1, int V, int blank, void* workspace, float* costs,
                           const float* shift_cur, float* shift_next, const float* emis, int* flag, void* stream);
int ttmi_rnnt_shift_seed(const void* workspace /* of a plain ttmi_rnnt_loss_fwd */, const int* act_lens, const int* label_lens, int B, int T,
                         int U1, float* shift_next, void* stream);
int ttmi_rnnt_loss_bwd_exp(void* P, long ldv, const int* labels, const int* act_lens, const int* label_lens, int B, int T, int U1,
                           int V, int blank, const void* workspace, const float* grad_out, int grad_out_stride, float scale,
                           float* srow, void* srow16, void* stream);

/* ---- FastEmit latency regularisation (Yu et al., ICASSP 2021) on the three loss backwards ----------------------------------------------
 * The _fe entry points take the arguments of ttmi_rnnt_loss_bwd / _bwd_split / _bwd_exp plus fastemit_lambda (finite, >= 0; anything else
 * is TTMI_EINVAL with a ttmi_last_error message).  The three entry points above are the _fe ones with fastemit_lambda = 0, bit for bit.
 * The costs (ttmi_rnnt_loss_fwd*) do not change: they stay -log P(y|x).  Per lattice cell (t, u) of utterance b, with lp = log_softmax(z),
 * ll = log P(y|x), occ = exp(alpha + beta - ll), e_l = exp(alpha(t,u) + lp(t,u,y_{u+1}) + beta(t,u+1) - ll) for u < U_b (0 otherwise) and
 * e_b the same for blank (beta(t+1,u); the terminal term at the last cell), g = scale * grad_out[b * grad_out_stride]:
 *     d z[k] = g * ( softmax_k * (occ + fastemit_lambda * e_l) - [k == blank] * e_b - [k == y_{u+1}] * (1 + fastemit_lambda) * e_l )
 * i.e. the plain gradient w.r.t. lp with its label-emission entries scaled by (1 + fastemit_lambda), chained through log_softmax (the
 * gradient-side form of NeMo's and other transducer losses).  Every row still sums to zero.  The exp-domain form changes only its per-row
 * factor srow (times 1 + fastemit_lambda * e_l / occ) and the blank / label entries it patches in P; its consumers are unchanged.
 * fastemit_lambda is a by-value kernel argument: a captured graph replays the value it was captured with. */
int ttmi_rnnt_loss_bwd_fe(const void* logits, int dtype, long ldv, const int* labels, const int* act_lens, const int* label_lens,
                          int B, int T, int U1, int V, int blank, const void* workspace, const float* grad_out,
                          int grad_out_stride, float scale, void* grad, long ldg, float fastemit_lambda, void* stream);
int ttmi_rnnt_loss_bwd_split_fe(void* logits, long ldv, const int* labels, const int* act_lens, const int* label_lens, int B, int T, int U1,
                                int V, int blank, const void* workspace, const float* grad_out, int grad_out_stride, float scale,
                                float fastemit_lambda, void* stream);
int ttmi_rnnt_loss_bwd_exp_fe(void* P, long ldv, const int* labels, const int* act_lens, const int* label_lens, int B, int T, int U1,
                              int V, int blank, const void* workspace, const float* grad_out, int grad_out_stride, float scale,
                              float* srow, void* srow16, float fastemit_lambda, void* stream);
int ttmi_joint_bwd_exp(const void* P, long ldg, const float* srow, const void* srow16, const float* enc, const float* dec,
                       const float* wf, const float* wp, int B, int T, int U1, int de, int dd, int J, int V, int prec, float* ctx,
                       float* ws, float* denc, float* ddec, float* g_wf, float* g_bf, float* g_wp, float* g_bp, void* stream);

/* ---- forced alignment and emission-time statistics (no reference counterpart: the reference's warprnnt_pytorch returns costs only) ------
 * Both read the workspace a finished ttmi_rnnt_loss_fwd OR ttmi_rnnt_loss_fwd_exp left on the same (B, T, U1) (either forward fills the
 * blank / label log-probs lpb / lpl, alpha, beta and ll).  The loss workspace is READ-ONLY here: a backward issued after an align / emit_stats
 * call gives the same bits as one issued straight after the forward.  Lengths are clamped as in the loss (T_b to [1, T], U_b to [0, U1-1]).
 * ttmi_rnnt_align: the best path.  v(0,0) = 0, v(t,u) = max(v(t-1,u) + lpb(t-1,u), v(t,u-1) + lpl(t,u-1)) for 0 <= t < T_b, 0 <= u <= U_b;
 * score[b] (f32) = v(T_b-1, U_b) + lpb(T_b-1, U_b), the log-probability of that path.  TIE RULE: the label move is taken only when it is
 * strictly greater; a tie goes to blank.  frames i32 [B, U1-1]: frames[b][u] = the frame t at which label u+1 is emitted (the path's move
 * (t, u) -> (t, u+1)), non-decreasing in u, -1 for u >= U_b.  The frontier is carried in fp64 like alpha / beta.  One decision bit per cell:
 * kept in LDS when an utterance's (T + U1 - 1) * ceil(U1 / 64) 8-byte words fit (128 KB), otherwise in align_workspace
 * (ttmi_rnnt_align_workspace_bytes(B, T, U1) bytes, 8-byte aligned, always required, contents undefined afterwards).
 * ttmi_set_option(23, bits) - measurements / tests only: 1 = decision words in align_workspace whatever the shape, 2 = no backtrace.
 * ttmi_rnnt_emit_stats: e(t,u) = exp(alpha(t,u) + lpl(t,u) + beta(t,u+1) - ll) for u < U_b is the posterior probability that label u+1 is
 * emitted at frame t; mass f32 [B, U1-1] = sum_t e(t,u) (1 for a healthy lattice: every alignment emits every label once), expected f32
 * [B, U1-1] = sum_t t e(t,u), the expected emission frame.  Entries u >= U_b: mass 0, expected -1.
 * Neither call synchronises with the host or issues a memset; both may be captured in a HIP graph.  U1 <= 1024 as for the loss. */
size_t ttmi_rnnt_align_workspace_bytes(int B, int T, int U1);
int ttmi_rnnt_align(const void* workspace /* filled by ttmi_rnnt_loss_fwd or _fwd_exp on the same (B,T,U1) */,
                    const int* act_lens, const int* label_lens, int B, int T, int U1,
                    void* align_workspace, int* frames, float* score, void* stream);
int ttmi_rnnt_emit_stats(const void* workspace, const int* act_lens, const int* label_lens, int B, int T, int U1,
                         float* expected, float* mass, void* stream);

/* ---- CTC loss and greedy decode for an auxiliary head on the audio encoder (joint CTC - transducer training; no reference counterpart) ----
 * logits f32 [B, T, V], batch-major, row pitch ldv >= V; labels i32 [B, U] (the tensor the RNN-T loss takes); act_lens, label_lens i32 [B],
 * clamped as in the RNN-T loss (T_b to [1, T], U_b to [0, U]); labels clamped to [0, V-1]; U <= 1023.  For utterance b the extended sequence
 * l' has S = 2 U_b + 1 entries, l'_{2k} = blank, l'_{2k+1} = y_k (built literally: a label equal to `blank` is not rejected), and
 * lp(t, s) = log_softmax(z[b, t])[l'_s].
 *     alpha(0, 0) = lp(0, 0), alpha(0, 1) = lp(0, 1), alpha(t, s) = lp(t, s) + logsumexp(alpha(t-1, s), alpha(t-1, s-1), alpha(t-1, s-2)),
 *     the s-2 term only when l'_s != blank and l'_s != l'_{s-2};  ll = logsumexp(alpha(T_b-1, S-1), alpha(T_b-1, S-2));  costs[b] = -ll;
 *     beta(T_b-1, S-1) = lp(T_b-1, S-1), beta(T_b-1, S-2) = lp(T_b-1, S-2), beta(t, s) = lp(t, s) + logsumexp(beta(t+1, s), beta(t+1, s+1),
 *     beta(t+1, s+2)), the s+2 term only when l'_{s+2} != blank and l'_{s+2} != l'_s  (beta includes the emission at t).
 * Alpha and beta are carried in fp64.  ttmi_ctc_loss_bwd, with g = scale * grad_out[b * grad_out_stride]:
 *     d z[b, t, k] = g * ( softmax_k - sum over {s : l'_s = k} of exp(alpha(t, s) + beta(t, s) - lp(t, s) - ll) )   for t < T_b
 * (every such row sums to zero), rows t >= T_b all zero, columns [V, ldg) zero; grad may alias logits when ldg == ldv.  The sum over the
 * states of one symbol has one owner and a fixed order (no floating-point atomics): two runs give the same bits.  An utterance with no
 * feasible alignment (fewer frames than labels plus adjacent repeats) has costs[b] = +inf and all-zero gradient rows, never NaN.
 * workspace: ttmi_ctc_workspace_bytes(B, T, U) bytes, 16-byte aligned; the forward fills it (emission table, alpha, beta, ll, log-sum-exp,
 * symbol chains), the backward reads it.  No allocation, host synchronisation or memset node: all three calls may be captured in a HIP graph.
 * ttmi_ctc_greedy: the argmax of each of the first T_b frames, repeats collapsed, blanks dropped -> tokens[b, :count[b]] (the rest of the
 * row is undefined).  The argmax order is the transducer scans' (NaN largest, ties to the lower index, always an index in [0, V)); if a
 * frame's maximum is not finite (NaN, +inf, or an all -inf row) count[b] = -(1 + the first such frame) instead of a count. */
size_t ttmi_ctc_workspace_bytes(int B, int T, int U);
int ttmi_ctc_loss_fwd(const float* logits, long ldv, const int* labels, const int* act_lens, const int* label_lens,
                      int B, int T, int U, int V, int blank, void* workspace, float* costs, void* stream);
int ttmi_ctc_loss_bwd(const float* logits, long ldv, const int* labels, const int* act_lens, const int* label_lens,
                      int B, int T, int U, int V, int blank, const void* workspace, const float* grad_out,
                      int grad_out_stride, float scale, float* grad, long ldg, void* stream);
int ttmi_ctc_greedy(const float* logits, long ld, const int* act_lens, int B, int T, int V, int blank,
                    int* tokens /* [B, T] */, int* count /* [B] */, void* stream);

/* ---- forced alignment and emission statistics on the CTC lattice (no reference counterpart) ---------------------------------------------
 * The twins of ttmi_rnnt_align / _emit_stats and ttmi_mono_align / _emit_stats on the lattice of the auxiliary head.  Both READ the workspace
 * a finished ttmi_ctc_loss_fwd left on the same (B, T, U) - lp, alpha, beta, ll - and write nothing into it: a ttmi_ctc_loss_bwd issued after
 * them gives the same bits as one issued straight after the forward.  Lengths and labels are clamped as in ttmi_ctc_loss_fwd, the extended
 * sequence l' (S = 2 U_b + 1 states) is built literally in the same way, and the skip rule is the loss's: the s-2 move only when
 * l'_s != blank and l'_s != l'_{s-2} - hence labels, label_lens, V and blank beside the workspace.
 * ttmi_ctc_align: the best path, frontier in fp64 like alpha; lp is the workspace's f32 table.
 *     v(0,0) = lp(0,0), v(0,1) = lp(0,1), every other state of frame 0 dead
 *     v(t,s) = lp(t,s) + max(v(t-1,s), v(t-1,s-1), v(t-1,s-2))            the s-2 term under the skip rule only
 * TIE RULE: predecessors are tried in the order s, s-1, s-2; a later one replaces an earlier one only when STRICTLY greater.  The path ends
 * in S-1 unless v(T_b-1, S-2) is strictly greater (U_b = 0: one state).  score f32 [B]: the log-probability of that path.  path i32 [B, T]:
 * the state index s at frame t < T_b, -1 for t >= T_b.  spans i32 [B, U, 2]: (first, last) frame on which the path sits in state 2u+1, so
 * first <= last < first of u+1; (-1, -1) for u >= U_b.  An utterance with no feasible alignment - best final value below the threshold that
 * makes the loss +inf - has score = -inf and every path and spans entry -1, never NaN; its neighbours are unaffected.  Whatever the
 * workspace holds, NaN included, the backtrace follows no index outside its arrays (s only decreases and is clamped at 0).
 * Decisions: one bit per blank state, two per label state (1.5 bits per cell), three 8-byte words per frame and 64 label positions; kept in
 * LDS when an utterance's T * ceil((U + 1) / 64) * 3 words fit 128 KB, otherwise in align_workspace (ttmi_ctc_align_workspace_bytes(B, T, U)
 * bytes, 8-byte aligned, always required, contents undefined afterwards).  ttmi_set_option(23, bits) is honoured as by ttmi_rnnt_align -
 * measurements / tests only: 1 = decision words in align_workspace whatever the shape, 2 = no backtrace (path entries t < T_b and spans
 * entries u < U_b are then not written).
 * ttmi_ctc_emit_stats: with s = 2u+1, g(t,s) = exp(alpha(t,s) + beta(t,s) - lp(t,s) - ll) is the posterior probability that frame t sits in
 * label u's state, and e(t,u) the posterior probability that label u's run STARTS at frame t:
 *     e(t,u) = exp(logsumexp(alpha(t-1,s-1), alpha(t-1,s-2) [skip rule]) + beta(t,s) - ll)   for t > 0  (beta includes the emission at t)
 *     e(0,0) = g(0,1),  e(0,u>0) = 0
 * mass f32 [B, U] = sum_t e(t,u) (1 for a healthy lattice: every alignment enters every label state exactly once), expected f32 [B, U] =
 * sum_t t e(t,u), the expected onset frame, duration f32 [B, U] = sum_t g(t, 2u+1), the expected number of frames the label occupies.
 * The sums are fp64, in frame order, by one owner; no floating-point atomics: two runs give the same bits.  Entries u >= U_b, and every
 * entry of an utterance with no feasible alignment: mass 0, expected -1, duration 0.
 * Neither call allocates, synchronises with the host or issues a memset node; both may be captured in a HIP graph.  rc < 0 with a
 * ttmi_last_error text, before any launch, on a null pointer (labels / spans / the statistics may be null when U = 0), B or T < 1, U < 0 or
 * U > 1023, V < 2, blank outside [0, V), a workspace that is not 16-byte aligned or an align_workspace that is not 8-byte aligned. */
size_t ttmi_ctc_align_workspace_bytes(int B, int T, int U);
int ttmi_ctc_align(const void* workspace /* filled by ttmi_ctc_loss_fwd on the same (B,T,U) */, const int* labels, const int* act_lens,
                   const int* label_lens, int B, int T, int U, int V, int blank, void* align_workspace,
                   int* path /* [B,T] */, int* spans /* [B,U,2] */, float* score /* [B] */, void* stream);
int ttmi_ctc_emit_stats(const void* workspace, const int* labels, const int* act_lens, const int* label_lens, int B, int T, int U, int V,
                        int blank, float* expected, float* mass, float* duration /* each [B,U] */, void* stream);

/* ---- CTC log-likelihood of hypotheses (N-best rescoring with the auxiliary head; no reference counterpart) -------------------------------
 * score f64 [P]: score[p] = log P_ctc(hyp[p] | logits[utt(p)]), the full sum over alignments, for P (hypothesis, utterance) pairs that SHARE
 * the utterances' logits: nothing is expanded per hypothesis, no emission table and no alpha is stored.
 * logits f32 [B, T, V], row pitch ldv >= V; act_lens i32 [B], clamped to [1, T].  hyp i64 [P, ld_hyp] (a beam's token histories go in as they
 * are), tokens clamped to [0, V-1]; hyp_len i32 [P], clamped to [0, U], U <= 1023 and U <= ld_hyp.  utt i32 [P] = the utterance of pair p,
 * clamped to [0, B-1]; utt = NULL: P must be a multiple of B and pair p belongs to utterance p / (P / B) (the beam's [B, W] layout).
 * The rule is ttmi_ctc_loss_fwd's, term for term and in its order: l' built literally (a token equal to `blank` is one more blank state),
 * lp(t, s) = max(-1e30, z[b,t,l'_s] - lse[b,t]) with the same row walk for lse, the alpha recursion above in fp64 with the same log-add-exp
 * order, the s-2 move only when l'_s != blank and l'_s != l'_{s-2}; score[p] = logsumexp(alpha(T_b-1, S-1), alpha(T_b-1, S-2)).  float(-score[p])
 * has the bits of costs[p] of a ttmi_ctc_loss_fwd on the gathered [P, T, V] batch when every gathered row keeps its address modulo 16 (the
 * row walk adds a row up from its first 16-byte boundary: another phase, another order, another last bit); where that cost is +inf (no
 * feasible alignment: fewer frames than tokens plus adjacent repeats) score[p] = -inf; a NaN stays a NaN.  A pair never affects another pair.
 * Two launches: the log-sum-exp of every row t < T_b once per utterance into `workspace` (ttmi_ctc_score_ws_bytes(B, T) bytes, 16-byte
 * aligned, contents undefined afterwards), then one workgroup per pair over all T_b frames (U + 1 <= 64: one wave).  No allocation, host
 * synchronisation, memset node or atomics; capturable in a HIP graph; two runs give the same bits; whatever the arrays hold, no index leaves
 * an array.  rc < 0 with a ttmi_last_error text, before any launch, on a null pointer (hyp may be null when U = 0; utt may be null), B, T or
 * P < 1, V < 2, blank outside [0, V), U < 0, U > 1023 or U > ld_hyp, ldv < V, utt = NULL with P % B != 0, a workspace that is not 16-byte
 * aligned or a score pointer that is not 8-byte aligned. */
size_t ttmi_ctc_score_ws_bytes(int B, int T);
int ttmi_ctc_score_hyps(const float* logits, long ldv, const int* act_lens, int B, int T, int V, int blank,
                        const long* hyp /* i64 [P, ld_hyp] */, long ld_hyp, const int* hyp_len /* [P] */,
                        const int* utt /* i32 [P] or NULL */, int P, int U,
                        void* workspace, double* score /* f64 [P] */, void* stream);

/* ---- monotonic RNN-T loss (Tripathi et al. 2019, "Monotonic RNN-T"; no reference counterpart) --------------------------------------------
 * The forward-backward over the lattice the decoders of this library walk (ttmi_greedy_*, ttmi_beam_step[_ctx]): every frame makes exactly
 * ONE decision, blank or one label, and the emitting frame is consumed - where the standard lattice above lets a label keep its frame.
 * Arguments as for ttmi_rnnt_loss_fwd / _bwd: logits [B,T,U1,V] (dtype 0 = f32, 1 = bf16), row pitch ldv >= V; labels i32 [B,U1-1], clamped
 * to [0, V-1]; act_lens, label_lens i32 [B], clamped as in the RNN-T loss (T_b to [1, T], U_b to [0, U1-1]); blank in [0, V); U1 <= 1024.
 * With lp = log_softmax(z[b,t,u,:]), lpb(t,u) = lp[blank], lpl(t,u) = lp[y_{u+1}] for u < U_b:
 *     alpha(0,0) = 0, alpha(0,u>0) = -inf
 *     alpha(t+1,u) = logaddexp(alpha(t,u) + lpb(t,u), alpha(t,u-1) + lpl(t,u-1))                 0 <= t < T_b, 0 <= u <= U_b
 *     ll = alpha(T_b, U_b),  costs[b] = -ll          (no terminal blank: after T_b decisions the path ends)
 *     beta(T_b,U_b) = 0, beta(T_b,u<U_b) = -inf
 *     beta(t,u) = logaddexp(lpb(t,u) + beta(t+1,u), lpl(t,u) + beta(t+1,u+1))
 * ttmi_mono_loss_bwd, with g = scale * grad_out[b * grad_out_stride], for t < T_b, u <= U_b:
 *     occ = exp(alpha(t,u) + beta(t,u) - ll)
 *     e_b = exp(alpha(t,u) + lpb(t,u) + beta(t+1,u) - ll)
 *     e_l = exp(alpha(t,u) + lpl(t,u) + beta(t+1,u+1) - ll)            (0 for u = U_b)
 *     d z[k] = g * ( softmax_k * occ - [k == blank] e_b - [k == y_{u+1}] e_l )
 * Every row sums to zero (occ = e_b + e_l).  A label equal to `blank` is not rejected: both patches then land on one column.  Rows outside
 * [0,T_b) x [0,U_b] are exact zeros, columns [V, ldg) are zeros; grad (the logits' dtype, pitch ldg) may alias logits when ldg == ldv.
 * An utterance with U_b > T_b has no path: costs[b] = +inf and all-zero gradient rows, never NaN (the rule of the CTC entries).
 * Alpha and beta are carried in fp64.  workspace: ttmi_mono_workspace_bytes(B, T, U1) bytes, 8-byte aligned, a layout of its own (NOT the
 * one ttmi_rnnt_align / _emit_stats read); the forward fills it, the backward reads it.  No allocation, host synchronisation, memset node
 * or floating-point atomic: both calls may be captured in a HIP graph, and two runs give the same bits. */
size_t ttmi_mono_workspace_bytes(int B, int T, int U1);
int ttmi_mono_loss_fwd(const void* logits, int dtype, long ldv, const int* labels, const int* act_lens, const int* label_lens,
                       int B, int T, int U1, int V, int blank, void* workspace, float* costs, void* stream);
int ttmi_mono_loss_bwd(const void* logits, int dtype, long ldv, const int* labels, const int* act_lens, const int* label_lens,
                       int B, int T, int U1, int V, int blank, const void* workspace, const float* grad_out,
                       int grad_out_stride, float scale, void* grad, long ldg, void* stream);

/* ---- token-and-duration transducer (TDT; Xu et al., ICML 2023; no reference counterpart) ---------------------------------------------------
 * The joint predicts a token AND the number of frames that decision consumes.  A row is z[b,t,u,0 : V+D] with pitch ldv >= V + D: V token
 * columns followed by D duration columns, each sub-row normalised by itself.  V is the TOKEN count.  durations: a HOST array of D entries,
 * copied into the launch: distinct integers in [1, 8], at most 8 of them, strictly increasing (no duration 0: every decoder here consumes
 * the emitting frame).  With durations = (1) this is the monotonic lattice above.  Other arguments as for ttmi_mono_loss_fwd / _bwd: dtype
 * 0 = f32, 1 = bf16; labels i32 [B,U1-1], clamped to [0, V-1]; act_lens, label_lens i32 [B], T_b clamped to [1, T], U_b to [0, U1-1]; blank
 * in [0, V); U1 <= 1024.  With lt = log_softmax(z[0:V]), ld = log_softmax(z[V:V+D]), lpb(t,u) = lt[blank], lpl(t,u) = lt[y_{u+1}] for
 * u < U_b, ld_j(t,u) = ld[j] the log-probability of durations[j] = d_j:
 *     alpha(0,0) = 0, everything else -inf
 *     alpha(t,u) = logsumexp over j with t - d_j >= 0 of   alpha(t-d_j, u)   + lpb(t-d_j, u)   + ld_j(t-d_j, u)
 *                                                          alpha(t-d_j, u-1) + lpl(t-d_j, u-1) + ld_j(t-d_j, u-1)    (u >= 1)
 *                                                                                              1 <= t <= T_b, 0 <= u <= U_b
 *     ll = alpha(T_b, U_b),  costs[b] = -ll
 *     beta(T_b,U_b) = 0;  beta(t,u) = logsumexp over j with t + d_j <= T_b of   lpb(t,u) + ld_j(t,u) + beta(t+d_j, u)
 *                                                                               lpl(t,u) + ld_j(t,u) + beta(t+d_j, u+1)   (u < U_b)
 * No terminal blank: a path is a sequence of decisions that lands EXACTLY on frame T_b.  A move that would overshoot (t + d_j > T_b) does
 * not exist in the lattice; its probability mass is lost, as in the published loss.
 * ttmi_tdt_loss_bwd, with g = scale * grad_out[b * grad_out_stride], for t < T_b, u <= U_b and each j with t + d_j <= T_b (0 otherwise):
 *     e_b,j = exp(alpha(t,u) + lpb + ld_j + beta(t+d_j, u)   - ll)
 *     e_l,j = exp(alpha(t,u) + lpl + ld_j + beta(t+d_j, u+1) - ll)         (0 for u = U_b)
 *     E_b = sum_j e_b,j   E_l = sum_j e_l,j   E_j = e_b,j + e_l,j   occ = E_b + E_l = exp(alpha(t,u) + beta(t,u) - ll)
 *     d z[k]     = g * ( softmax_tok[k] * occ - [k == blank] E_b - [k == y_{u+1}] E_l )        0 <= k < V
 *     d z[V + j] = g * ( softmax_dur[j] * occ - E_j )                                          0 <= j < D
 * Both sub-rows sum to zero.  A label equal to `blank` is not rejected.  Rows outside [0,T_b) x [0,U_b] are exact zeros, columns
 * [V+D, ldg) are zeros; grad (the logits' dtype, pitch ldg >= V + D) may alias logits when ldg == ldv.  An utterance with no path - U_b > T_b,
 * or T_b not a sum of durations (durations = (2) with an odd T_b) - has costs[b] = +inf and all-zero gradient rows, never NaN; its
 * neighbours are unaffected.  Alpha and beta are carried in fp64 in a fixed summation order (alpha: by source frame; beta: j ascending).
 * workspace: ttmi_tdt_workspace_bytes(B, T, U1, D) bytes, 8-byte aligned; the forward fills it, the backward reads it.  No allocation, host
 * synchronisation, memset node or floating-point atomic: both calls may be captured in a HIP graph, and two runs give the same bits.
 * rc < 0 with a ttmi_last_error text, before any launch, on a null pointer, a shape outside the limits, D outside [1,8], a duration outside
 * [1,8] or durations not strictly increasing, ldv (or ldg) < V + D.
 * NOT built on this lattice: the exp-domain form, FastEmit, alignment / emission statistics, distillation, beam search.
 *
 * Greedy decoding, the lockstep-over-symbol-steps pair of ttmi_greedy_scan_batch_lp / ttmi_greedy_advance_lp with jumps.  Per utterance, at
 * frame t against the current label state: k* = argmax z[0:V], j* = argmax z[V:V+D] (in both the LOWEST index wins a tie and a NaN counts as
 * the largest value: the order of ttmi_greedy_scan_batch), d = durations[j*], the decision's log-probability is lt[k*] + ld[j*].  Blank:
 * t += d.  Token: k* is emitted on frame t, then t += d and the label state advances.  The utterance ends when t >= T_len[b] (the decoder
 * may overshoot: it then ends).
 * ttmi_tdt_scan_batch: logits [B, n, V+D] (row pitch ld >= V + D) = the joint of frames t[b] .. t[b] + n - 1 of every utterance against its
 * own label state.  For every row that exists (need[b] != 0, t[b] + r < T_len[b]): dec[b][r] = (k*, j*) (device i32 [B, n, 2]),
 * lp[b][r] = (lt[k*], ld[j*]) (device f32 [B, n, 2]), one pass per sub-row in f32 (bf16 widened exactly); NaN where the sub-row's
 * log-sum-exp is not finite.  Other rows are NOT written.
 * ttmi_tdt_advance: one thread per utterance with need[b] follows the jumps through the block from row 0, t0 = t[b]: the decision of row r
 * adds lp[b][r][0] + lp[b][r][1] to score[b] (device f64 [B], zeroed by the caller before the first block; one thread, row order: the same
 * bits in every run) and moves r on by d.  It stops at the first token - hist[b][n_hist] = k*, frames[b][c] = t0 + r, tok_lp[b][c] =
 * lt[k*], tok_dur[b][c] = d at c = count[b] (i32 / f32 / i32 [B, ld_det], count[b] < ld_det required), count[b] += 1, need[b] = 0 - or when
 * the jump leaves the block or the utterance.  A jump that leaves the block CARRIES OVER: t[b] becomes t0 + r exactly, not t0 + n.  Once
 * t[b] >= T_len[b]: need[b] = 0, done[b] = 1 (also straight after a token).  Utterances with need[b] == 0 are left alone.  flags[0] =
 * utterances that still need a symbol in this step, flags[1] = utterances not finished, as ttmi_greedy_advance leaves them (written, not
 * added: nothing is zeroed first).  `durations` is a HOST array as above.  Neither call allocates, synchronises with the host or issues a
 * memset node; both may be captured in a HIP graph. */
size_t ttmi_tdt_workspace_bytes(int B, int T, int U1, int D);
int ttmi_tdt_loss_fwd(const void* logits, int dtype, long ldv, const int* labels, const int* act_lens, const int* label_lens,
                      int B, int T, int U1, int V, int blank, const int* durations, int D, void* workspace, float* costs, void* stream);
int ttmi_tdt_loss_bwd(const void* logits, int dtype, long ldv, const int* labels, const int* act_lens, const int* label_lens,
                      int B, int T, int U1, int V, int blank, const int* durations, int D, const void* workspace, const float* grad_out,
                      int grad_out_stride, float scale, void* grad, long ldg, void* stream);
int ttmi_tdt_scan_batch(const void* logits, int dtype, long ld, int B, int n, int V, int D, const int* t, const int* T_len,
                        const int* need, int* dec, float* lp, void* stream);
int ttmi_tdt_advance(const int* dec, const float* lp, int B, int n, int blank, const int* durations, int D, int n_hist, long* hist,
                     long ld_hist, int* t, const int* T_len, int* need, int* done, int* count, int* flags, int* frames, float* tok_lp,
                     int* tok_dur, long ld_det, double* score, void* stream);

/* ---- forced alignment and emission-time statistics on the monotonic lattice (no reference counterpart) ---------------------------------
 * The twins of ttmi_rnnt_align / _emit_stats on the lattice above.  Both READ the workspace a finished ttmi_mono_loss_fwd left on the same
 * (B, T, U1) - lpb, lpl, alpha, beta, ll - and write nothing into it: a ttmi_mono_loss_bwd issued after them gives the same bits as one
 * issued straight after the forward.  Lengths are clamped as in the loss (T_b to [1, T], U_b to [0, U1-1]); U1 <= 1024.
 * ttmi_mono_align: the best path, frontier in fp64 like alpha / beta.
 *     v(0,0) = 0, v(0,u>0) = -inf
 *     v(t+1,u) = max(v(t,u) + lpb(t,u), v(t,u-1) + lpl(t,u-1))                                     0 <= t < T_b, 0 <= u <= U_b
 *     score[b] = (float) v(T_b, U_b)                  (no terminal blank), the log-probability of that path
 * TIE RULE: the label move is taken only when it is strictly greater; a tie goes to blank.  The backtrace runs from (T_b, U_b) backwards in
 * time, so on all-equal logits it yields frames = 0, 1, ..., U_b-1.  frames i32 [B, U1-1]: frames[b][u] = the frame whose one decision is
 * label u+1 (the path's move (t, u) -> (t+1, u+1)), STRICTLY increasing in u (ttmi_rnnt_align's is only non-decreasing), -1 for u >= U_b.
 * This is the lattice of ttmi_greedy_advance_lp's and ttmi_beam_step's scores: score[b] is an upper bound of the score of any decoder path
 * that spells the same labels.  An utterance with U_b > T_b has no path: score[b] = -inf and every frames entry -1, never NaN; its
 * neighbours are unaffected.  Whatever the workspace holds, NaN included, the backtrace follows no index outside its arrays and writes
 * nothing outside the utterance's frames row: with u labels left at frame t it keeps u <= t + 1 (the move is a label whatever the stored
 * bit says once u = t + 1, a blank once u = 0).  One decision bit per cell: kept in LDS when an utterance's T * ceil(U1 / 64) 8-byte words
 * fit (128 KB), otherwise in align_workspace (ttmi_mono_align_workspace_bytes(B, T, U1) bytes, 8-byte aligned, always required, contents
 * undefined afterwards).  ttmi_set_option(23, bits) is honoured as by ttmi_rnnt_align - measurements / tests only: 1 = decision words in
 * align_workspace whatever the shape, 2 = no backtrace.
 * ttmi_mono_emit_stats: e(t,u) = exp(alpha(t,u) + lpl(t,u) + beta(t+1,u+1) - ll) for u < U_b, t < T_b is the posterior probability that
 * label u+1 is frame t's decision; mass f32 [B, U1-1] = sum_t e(t,u) (1 for a healthy lattice: every path emits every label once), expected
 * f32 [B, U1-1] = sum_t t e(t,u), the expected emission frame.  Entries u >= U_b: mass 0, expected -1; an utterance without a path: mass 0
 * and expected -1 in every entry.  The sums are fp64 in a fixed order, no floating-point atomics: two runs give the same bits.
 * Neither call allocates, synchronises with the host or issues a memset node; both may be captured in a HIP graph.  rc < 0 with a
 * ttmi_last_error text, before any launch, on a null pointer or a shape outside the limits. */
size_t ttmi_mono_align_workspace_bytes(int B, int T, int U1);
int ttmi_mono_align(const void* workspace /* filled by ttmi_mono_loss_fwd on the same (B,T,U1) */,
                    const int* act_lens, const int* label_lens, int B, int T, int U1,
                    void* align_workspace, int* frames, float* score, void* stream);
int ttmi_mono_emit_stats(const void* workspace, const int* act_lens, const int* label_lens, int B, int T, int U1,
                         float* expected, float* mass, void* stream);

/* ---- transducer knowledge distillation on collapsed lattice posteriors (Panchapagesan et al., ICASSP 2021; no reference counterpart) -----
 * The distribution of every lattice node over the V outputs is collapsed to three classes - blank, the next label y_{u+1}, everything else -
 * and the student is trained with the KL divergence from the teacher's three probabilities to its own.  The teacher hands over three floats
 * per node instead of V logits, and need not share the student's V.  Arguments as for ttmi_mono_loss_fwd / _bwd: logits [B,T,U1,V] (dtype
 * 0 = f32, 1 = bf16), row pitch ldv >= V; labels i32 [B,U1-1], clamped to [0, V-1]; act_lens, label_lens i32 [B], T_b clamped to [1, T],
 * U_b to [0, U1-1]; blank in [0, V); V >= 2.  For a node (t, u), t < T_b, u <= U_b, with s = softmax(z[b,t,u,:]) and y = labels[b][u]; the
 * label class is EMPTY when u == U_b or y == blank:
 *     lb = z[blank] - lse          ly = z[y] - lse (NEG = -1e30 for an empty label class)          lo = lse(z[k], k not in {blank, y}) - lse
 * lo is a log-sum-exp of its own over the other columns, taken in the same online pass; the row's lse is that sum joined with the two columns
 * left out.  It is never formed as 1 - p_b - p_y, which loses the other mass of a confident row to cancellation.  Every collapsed
 * log-probability is clamped below at NEG; an empty class holds NEG.
 * ttmi_kd_collapse (the teacher's call): post f32 [B,T,U1,3] = (lb, ly, lo); rows outside the ragged lattice are exact zeros.
 * ttmi_kd_loss_fwd (the student's): teacher f32 [B,T,U1,3] as ttmi_kd_collapse wrote it - the caller's contract is entries <= 0, or NEG for
 * an empty class; P^T_c = exp(teacher_c), and P^T_y is taken as 0 where the student's label class is empty.
 *     kd(t,u)  = sum_c P^T_c (log P^T_c - log P^S_c)                a class with P^T_c == 0 adds exactly 0
 *     costs[b] = sum of kd over the utterance's nodes, fp64, in an order fixed by the shape (a second small launch), no atomics
 * A NaN teacher entry makes its utterance's cost NaN; no index depends on a teacher value.  Per row the workspace keeps one 16-byte record
 * (lse, c_o, P^T_b, P^T_y), c_o = P^T_o / P^S_o = exp(teacher_o - lo), 0 when the other class is empty on either side, and one f32 row cost.
 * ttmi_kd_loss_bwd, with g = scale * grad_out[b * grad_out_stride]:
 *     d z[k] = g * ( s_k - P^T_b )             k == blank
 *              g * ( s_k - P^T_y )             k == y, label class not empty
 *              g * s_k (1 - c_o)               otherwise
 * Every row sums to zero when the teacher's three probabilities sum to one.  accumulate = 0: grad (the logits' dtype, pitch ldg) is written;
 * rows outside the lattice and columns [V, ldg) are zeros; grad may alias logits when ldg == ldv.  accumulate = 1: the gradient is ADDED to
 * what grad holds, over the lattice's rows and columns [0, V) - widened to f32, added, rounded once - and no other byte of grad is touched;
 * aliasing the logits is TTMI_EINVAL.  workspace: ttmi_kd_workspace_bytes(B, T, U1) bytes, 16-byte aligned; the forward fills it, the
 * backward reads it.  One wave per row, the 16-byte row walk of the monotonic loss, any pitch >= V.  No allocation, host synchronisation,
 * memset node or floating-point atomic: every call may be captured in a HIP graph, and two runs give the same bits.  rc < 0 with a
 * ttmi_last_error text, before any launch, on a null pointer or V < 2. */
size_t ttmi_kd_workspace_bytes(int B, int T, int U1);
int ttmi_kd_collapse(const void* logits, int dtype, long ldv, const int* labels, const int* act_lens, const int* label_lens,
                     int B, int T, int U1, int V, int blank, float* post /* [B,T,U1,3] */, void* stream);
int ttmi_kd_loss_fwd(const void* logits, int dtype, long ldv, const int* labels, const int* act_lens, const int* label_lens,
                     int B, int T, int U1, int V, int blank, const float* teacher /* [B,T,U1,3] */, void* workspace, float* costs,
                     void* stream);
int ttmi_kd_loss_bwd(const void* logits, int dtype, long ldv, const int* labels, const int* act_lens, const int* label_lens,
                     int B, int T, int U1, int V, int blank, const void* workspace, const float* grad_out,
                     int grad_out_stride, float scale, void* grad, long ldg, int accumulate, void* stream);

/* ---- grouped weight gradients (data-parallel hot path): the four weight-gradient GEMMs of an encoder layer are a quarter
 * of the chip each step; deferred and launched four layers at a time they are 256 tiles, one per CU over the whole reduction - no split along
 * K, no atomics, bit-identical from run to run and across ranks.  ttmi_attn_bwd_defer / ttmi_ffn_bwd_defer are ttmi_attn_bwd / ttmi_ffn_bwd
 * minus those GEMMs: the bf16 operands that would have lived in the scratch workspace go to `keep` (ttmi_*_keep_bytes; 256-byte aligned,
 * caller-owned until the group has run) and `out` receives the problems (2 per call) for ttmi_wgrad_group.  bf16 pipeline only (returns an
 * error otherwise: callers test ttmi_wgrad_defer_supported first). */
typedef struct ttmi_wgrad_desc {
    const void* A;      /* bf16 [K, M], row pitch lda */
    const void* B;      /* bf16 [K, N], row pitch ldb */
    float* C;           /* f32 [M, N], row pitch ldc: C += A^T B */
    float* colsum;      /* nullable, f32 [M]: += column sums of A */
    int M, N, K;
    long lda, ldb, ldc;
} ttmi_wgrad_desc;
int ttmi_wgrad_group(const ttmi_wgrad_desc* descs /* host array */, int n, void* stream);
int ttmi_wgrad_defer_supported(long rows, int d, int H, int Dh, int Di, int prec);
size_t ttmi_attn_bwd_keep_bytes(int B, int L, int d, int H, int Dh);
size_t ttmi_ffn_bwd_keep_bytes(long rows, int d, int Di);
int ttmi_attn_bwd_defer(const float* dy, const float* x, const float* qkv_w, const float* o_w, const float* ln_g,
                        const float* r_emb, const float* r_w_bias, const float* r_bias, int B, int L, int d, int H, int Dh, int K, int mask_kind,
                        int mask_left, int mask_right, const unsigned char* mask, long mask_sb, long mask_si, int prec,
                        float p_drop, unsigned seed, const float* ctx, float* ws, float* dx, float* g_qkv_w, float* g_o_w,
                        float* g_ln_g, float* g_ln_b, float* g_r_emb, float* g_r_w_bias, float* g_r_bias, void* keep,
                        ttmi_wgrad_desc* out /* 2 entries */, void* stream);
int ttmi_ffn_bwd_defer(const float* dz, const float* y, const float* w1, const float* w2, const float* ln_g, long rows, int d, int Di,
                       int prec, float p_drop, float p_layer, unsigned seed, const float* ctx, float* ws, float* dy, float* g_w1,
                       float* g_b1, float* g_w2, float* g_b2, float* g_ln_g, float* g_ln_b, void* keep,
                       ttmi_wgrad_desc* out /* 2 entries */, void* stream);

/* ---- one encoder layer per call: RelLearnableDecoderLayer.forward (tt/transformer.py:188-197) = ttmi_attn_fwd + ttmi_ffn_fwd, and
 * their backward, behind ONE entry each.  Where ttmi_layer_fused() is 1 (bf16 pipeline, d % 4 == 0, d <= 512) the calls share three passes
 * the sub-layer boundary forces apart: the FFN's pre-norm comes out of the attention sub-layer's post-norm pass, the two LayerNorm backward
 * passes that meet at y are one kernel (dy is never stored), and the bf16 copy of the layer's input is taken from its producer (x16_in: bf16
 * [B*L, d] or NULL; z16_out: bf16 [B*L, d] or NULL - hand a layer's z16_out to the next layer as x16_in, to forward AND backward).
 * Otherwise they run the sub-layer calls back to back.  ctx_attn / ctx_ffn: ttmi_attn_ctx_floats / ttmi_ffn_ctx_floats, saved for backward;
 * ws: ttmi_layer_ws_floats; y ([B, L, d], the attention sub-layer's output) is an output of forward and an input of backward.
 * ttmi_layer_bwd with keep_attn / keep_ffn / out (ttmi_*_bwd_keep_bytes; 4 descriptors: CoreNet.3, CoreNet.0, o_net, qkv_net) defers the
 * weight-gradient GEMMs as ttmi_*_bwd_defer do; all three NULL runs them here. */
int ttmi_layer_fused(int d, int H, int Dh, int Di, int prec);
size_t ttmi_layer_ws_floats(int B, int L, int d, int H, int Dh, int Di, int prec);
int ttmi_layer_fwd(const float* x, const void* x16_in, const float* qkv_w, const float* o_w, const float* ln_g, const float* ln_b, const float* r_emb,
                   const float* r_w_bias, const float* r_bias, const float* w1, const float* b1, const float* w2, const float* b2,
                   const float* ff_ln_g, const float* ff_ln_b, int B, int L, int d, int H, int Dh, int K, int Di, int mask_kind, int mask_left,
                   int mask_right, const unsigned char* mask, long mask_sb, long mask_si, int prec, float p_drop_attn, unsigned seed_attn,
                   float p_drop_ffn, float p_layer, unsigned seed_ffn, float* ctx_attn, float* ctx_ffn, float* ws, float* y, float* z,
                   void* z16_out, void* stream);
int ttmi_layer_bwd(const float* dz, const float* x, const void* x16_in, const float* y, const float* qkv_w, const float* o_w, const float* ln_g,
                   const float* r_emb, const float* r_w_bias, const float* r_bias, const float* w1, const float* w2, const float* ff_ln_g, int B,
                   int L, int d, int H, int Dh, int K, int Di, int mask_kind, int mask_left, int mask_right, const unsigned char* mask,
                   long mask_sb, long mask_si, int prec, float p_drop_attn, unsigned seed_attn, float p_drop_ffn, float p_layer,
                   unsigned seed_ffn, const float* ctx_attn, const float* ctx_ffn, float* ws, float* dx, float* g_qkv_w, float* g_o_w,
                   float* g_ln_g, float* g_ln_b, float* g_r_emb, float* g_r_w_bias, float* g_r_bias, float* g_w1, float* g_b1, float* g_w2,
                   float* g_b2, float* g_ff_ln_g, float* g_ff_ln_b, void* keep_attn, void* keep_ffn, ttmi_wgrad_desc* out /* 4 entries */,
                   void* stream);

/* ---- greedy decoding support (Transducer.decode, tt/model.py:70-90): logits rows = consecutive frames against one label
 * state; *out (device u64) = (first row whose argmax != blank) << 32 | symbol, or n << 32 if all rows are blank. */
int ttmi_greedy_scan(const void* logits, int dtype, long ld, int n, int V, int blank, unsigned long long* out, void* stream);
/* Batched greedy decoding (tt/model.py:92-108 recognize -> decode for every utterance), all utterances of a batch in lockstep over SYMBOL steps:
 * after step s every utterance still decoding holds exactly s + 1 tokens, so one label-encoder call of length s + 1 serves the batch exactly.
 * ttmi_greedy_scan_batch: logits [B, n, V] (row pitch ld) = the joint of frames t[b] .. t[b] + n - 1 of every utterance against its own label state;
 * key[b] (device u64, n << 32 before the call) = min over the utterance's frames that exist (t[b] + r < T_len[b]) and whose argmax is not `blank`
 * of (r << 32 | symbol); utterances with need[b] == 0 are left alone.  ttmi_greedy_advance consumes key: symbol found -> hist[b][n_hist] =
 * symbol, t[b] += r + 1, count[b] += 1, need[b] = 0; none -> t[b] += n, and need[b] = 0, done[b] = 1 once t[b] >= T_len[b]; key is reset;
 * flags[0] = utterances that still need a symbol in this step, flags[1] = utterances not finished (one 8-byte read per scan for the host). */
int ttmi_greedy_scan_batch(const void* logits, int dtype, long ld, int B, int n, int V, int blank, const int* t, const int* T_len,
                           const int* need, unsigned long long* key, void* stream);
int ttmi_greedy_advance(unsigned long long* key, int B, int n, int n_hist, long* hist, long ld_hist, int* t, const int* T_len, int* need,
                        int* done, int* count, int* flags, void* stream);
/* The same pair with what the scan's logits also say about each decision (Transducer.decode_batch(details=True)): where every token was
 * emitted, how probable it was, and the log-probability of the whole greedy path.
 * ttmi_greedy_scan_batch_lp: ttmi_greedy_scan_batch (same rows skipped, key bit-identical) that also writes lp (device f32 [B, n, 2]) for every
 * row it walks: lp[b][r][0] = log P(blank) = x[blank] - lse, lp[b][r][1] = log P(argmax) = x[argmax] - lse, lse = the row's log-sum-exp, taken in
 * the same single pass over the row in f32 (bf16 logits widened exactly).  The two are equal when the argmax is the blank.  Rows the scan skips
 * (need[b] == 0, t[b] + r >= T_len[b]) are NOT written.  A row whose log-sum-exp is not finite (it holds a NaN or +inf, or is all -inf) gives NaN
 * in both entries; its key is ttmi_greedy_scan_batch's.  A `blank` outside [0, V) is a blank of probability 0: entry 0 = -inf.
 * ttmi_greedy_advance_lp: ttmi_greedy_advance (same transitions, same flags) that also, for every utterance with need[b], t0 = t[b] and
 * c = count[b] before the update: symbol found at row r -> frames[b][c] = t0 + r, tok_lp[b][c] = lp[b][r][1], score[b] += sum over r' < r of
 * lp[b][r'][0], + lp[b][r][1]; none -> score[b] += sum of lp[b][r'][0] over the rows with t0 + r' < T_len[b].  frames i32 / tok_lp f32
 * [B, ld_det], count[b] < ld_det required; score: device f64 [B], the caller zeroes it before the first block.  The sum is taken by the
 * utterance's one thread, in row order, in f64: no floating-point atomics, two runs give the same bits.
 * score[b] is the log-probability of the decisions the greedy decoder took: each of the utterance's T_b frames contributes one term, blank's
 * log-probability against the label state current at that frame on a frame that does not emit, the symbol's on a frame that does (the emitting
 * frame is consumed: at most one symbol per frame).  That is the path of this decoder, NOT a path of the RNN-T lattice (the lattice follows a
 * label with a blank on the same frame): it is not comparable with ttmi_rnnt_align's score.  It IS a path of the monotonic lattice: the
 * score ttmi_mono_align gives for the same labels is its upper bound, and equal to it when the two paths emit at the same frames.
 * Neither call allocates, synchronises with the host or issues a memset node; both may be captured in a HIP graph. */
int ttmi_greedy_scan_batch_lp(const void* logits, int dtype, long ld, int B, int n, int V, int blank, const int* t, const int* T_len,
                              const int* need, unsigned long long* key, float* lp, void* stream);
int ttmi_greedy_advance_lp(unsigned long long* key, int B, int n, int n_hist, long* hist, long ld_hist, int* t, const int* T_len, int* need,
                           int* done, int* count, int* flags, const float* lp, int* frames, float* tok_lp, long ld_det, double* score,
                           void* stream);
/* Frame-synchronous beam search on the greedy path's probability model (Transducer.beam_decode_batch): each of an utterance's frames takes
 * one decision, blank or one symbol, against the label state of the tokens so far; the emitting frame is consumed.  ttmi_beam_step takes the
 * beam of every utterance over ONE frame.  One workgroup per utterance; it allocates nothing, does not synchronise with the host, issues no
 * memset node and may be captured in a HIP graph.
 * In: logits [B, W, V] (dtype 0 = f32, 1 = bf16 widened exactly; row pitch ld >= V): row (b, w) = the joint of frame t[b] against the label
 * state of hypothesis w; blank in [0, V); t, T_len i32 [B]; the beam: score_in f64 [B, W], len_in i32 [B, W] (symbols emitted, the start symbol
 * not counted), hist_in i64 [B, W, ld_hist] (column 0 = the start symbol, columns 1 .. len = the symbols), and - all four or none -
 * frames_in i32 / tok_lp_in f32 [B, W, ld_det] (emission frame and log-probability of every symbol) with their _out twins.
 * Out, in buffers of their own (the caller swaps): score_out, len_out, hist_out (columns 0 .. len_out), frames_out / tok_lp_out (len_out
 * entries); parent i32 [B, W] = the slot of the old beam the new slot continues; fresh i32 [B, W] = 1 where the slot is its parent extended by
 * a symbol (it needs a new label state), 0 where it keeps its parent's tokens (and label state).
 * Limits: 1 <= W <= 32, V >= 2, ld_hist >= the largest len_in + 2 (ld_det >= the largest len_in + 1); the kernel never reads or writes past a
 * row, whatever len_in says.
 * Rule, per utterance with t[b] < T_len[b]:
 *  - lp(w, k) = x[w][k] - lse(row w), in one f32 pass over the row as ttmi_greedy_scan_batch_lp takes it; a row without a finite log-sum-exp
 *    (a NaN, a +inf, nothing but -inf) has lp = NaN throughout.
 *  - A slot whose score is -inf (or NaN) is empty: it extends nothing and takes part in no merge.
 *  - Candidates of every live slot i: its blank extension (tokens_i, score_i + lp(i, blank)) and its symbol extensions
 *    (tokens_i + k, score_i + lp(i, k)), k != blank; sums in f64.  A candidate score that is NaN counts as -inf.
 *  - Live slots hold distinct sequences (the caller's contract, kept by this rule), so two candidates spell the same sequence only as the blank
 *    extension of i and the extension of j by k with tokens_i = tokens_j + k.  Those two are ONE candidate: tokens_i, score = log(exp(a) +
 *    exp(b)) of the two in f64, counted as a blank extension (parent i, fresh 0); frames / tok_lp are those of whichever of the two had the
 *    larger score before the merge (the blank side's on a tie): i's own, or j's followed by (t[b], lp(j, k)).  The symbol side enters the merge
 *    wherever it would rank among j's symbols.
 *  - The new beam = the W best candidates under the total order: score descending, then parent slot ascending, then blank before symbols,
 *    then symbol ascending; selected by counting ranks under that order (no atomics on values: two runs give the same bits).  A symbol
 *    extension has parent i, fresh 1, len_i + 1 tokens and i's details followed by (t[b], lp(i, k)).  Only candidates with a score > -inf
 *    take a slot; slots left over are empty: score -inf, len 0, parent = the slot itself, fresh 0 (their hist / frames / tok_lp rows are not
 *    written).
 * An utterance with t[b] >= T_len[b] is finished: its beam is copied through, parent = identity, fresh = 0.  t is not advanced: the caller does.
 * A beam starts as slot 0 = (score 0, len 0, hist[0] = start symbol), every other slot empty. */
int ttmi_beam_step(const void* logits, int dtype, long ld, int B, int W, int V, int blank, const int* t, const int* T_len,
                   const double* score_in, const int* len_in, const long* hist_in, const int* frames_in, const float* tok_lp_in,
                   double* score_out, int* len_out, long* hist_out, int* frames_out, float* tok_lp_out, long ld_hist, long ld_det,
                   int* parent, int* fresh, void* stream);
/* Contextual biasing (hotword boosting) inside the beam step: ttmi_beam_step_ctx is ttmi_beam_step with a deterministic weighted automaton
 * over tokens steering the selection (ttmi.context.ContextGraph compiles one from hotword phrases; any automaton that meets the contract
 * fits, a back-off n-gram table too).  Same launch shape and promises: one workgroup per utterance, no allocation, no host synchronisation,
 * no memset node, capturable in a HIP graph, no floating-point atomics, two runs give the same bits.
 * The automaton, device arrays: S >= 1 states, state 0 the root; A >= 0 arcs.  arc_off i32 [S + 1]; arc_sym / arc_next i32 [A], arc_w f32 [A]:
 * the arcs of state s are entries arc_off[s] .. arc_off[s + 1] - 1, their symbols strictly ascending within a state and never the blank.
 * fail i32 [S] with fail[s] < s for s > 0 (a failure chain ends at the root in at most S hops); fail_w f32 [S], fail_w[0] = the weight of a
 * symbol without an arc at the root (it stays at the root).  All weights finite.  (A final weight per state is the host's business.)
 * Transition step(s, k) -> (s', delta), delta accumulated in f64 in exactly this order:
 *     acc = 0.0
 *     loop: if s has an arc on k:  return (arc_next, acc + (double)arc_w)
 *           if s == 0:             return (0, acc + (double)fail_w[0])
 *           acc += (double)fail_w[s]; s = fail[s]
 * State and accumulated bias are functions of the token sequence alone, so the two sides of a merge always carry the same state and the
 * same bias bits: the merge rule needs no new case.
 * Arguments: ttmi_beam_step's, then S, A and the six tables, then per slot state_in i32 [B, W] and bias_in f64 [B, W] with their _out twins
 * in buffers of their own, then ws: ttmi_beam_ctx_ws_bytes(B, W, V) bytes of device memory the kernel may overwrite (B * W * V f64: per live
 * slot the row of finished biases bias + delta(state, k) of every symbol k, written once per frame by the row's own wave, so that the
 * candidate passes add one number per symbol and follow no chain).  It carries nothing from call to call.
 * Rule = ttmi_beam_step's rule with these changes and no others:
 *  - Every candidate has a score (unchanged: the model's log-probability, f64, merged by log-sum), a bias and a state.  The blank extension
 *    of i: bias_i, state_i.  The extension of i by k: (state', delta) = step(state_i, k), bias' = bias_i + delta.
 *  - key = score + bias', the f64 sum of the finished score and the finished bias; a NaN key counts as -inf.  The total order, the
 *    per-parent preselection of the W best symbols and the rank counting use the key where ttmi_beam_step uses the score; the tie-break is
 *    unchanged (parent ascending, blank before symbols, symbol ascending).  A candidate takes a slot only if its score > -inf and its key > -inf.
 *  - A merged candidate takes i's state and bias; which side's details it takes is decided by the two SCORES, as in ttmi_beam_step.
 *  - A state_in outside [0, S) is read as the root.  Whatever the tables hold, no index is followed outside them (an arc range is clamped
 *    to [0, A], a failure link outside [0, S) reads as the root, a chain is left after S hops, an arc symbol outside [0, V) is ignored).
 *  - A finished utterance (t[b] >= T_len[b]) copies state and bias through; an empty new slot gets state 0 and bias 0.
 * score_out stays the model's log-probability.  With all weights zero every output ttmi_beam_step also has is bit-identical to its.
 * rc < 0 with a ttmi_last_error text before any launch on a null pointer (the arc arrays may be null when A == 0), S < 1, A < 0, an _out
 * buffer that is its _in buffer, or anything ttmi_beam_step refuses. */
size_t ttmi_beam_ctx_ws_bytes(int B, int W, int V);
int ttmi_beam_step_ctx(const void* logits, int dtype, long ld, int B, int W, int V, int blank, const int* t, const int* T_len,
                       const double* score_in, const int* len_in, const long* hist_in, const int* frames_in, const float* tok_lp_in,
                       double* score_out, int* len_out, long* hist_out, int* frames_out, float* tok_lp_out, long ld_hist, long ld_det,
                       int* parent, int* fresh, int S, int A, const int* arc_off, const int* arc_sym, const int* arc_next, const float* arc_w,
                       const int* fail, const float* fail_w, const int* state_in, const double* bias_in, int* state_out, double* bias_out,
                       void* ws, void* stream);
/* Language-model fusion inside the beam step: ttmi_beam_step_fuse is ttmi_beam_step_ctx with dense external scores, the rows a neural
 * language model (shallow fusion) or the label encoder's own prior (internal-LM subtraction) gives for every hypothesis.  Same launch shape
 * and promises: one workgroup per utterance, no allocation, no host synchronisation, no memset node, capturable in a HIP graph, no
 * floating-point atomics, two runs give the same bits.
 * Arguments: ttmi_beam_step_ctx's, automaton included (a search without hotwords passes the trivial one: S = 1, A = 0, arc_off = {0, 0},
 * fail = {0}, fail_w = {0}); ws holds ttmi_beam_fuse_ws_bytes(B, W, V) bytes.  Then the per-slot accumulator fuse_in / fuse_out f64 [B, W] in
 * buffers of their own, double sym_bonus, and up to two sources j in {0, 1}: ext_j (device pointer, NULL = absent), ext_j_dtype (0 = f32,
 * 1 = bf16), ext_j_ld >= V (row (b, w) starts at element (b * W + w) * ext_j_ld), double ext_j_w, int ext_j_norm.  Row (b, w) of a source
 * belongs to the hypothesis of slot w and is a function of that slot's tokens alone, so the two sides of a merge carry the same fuse.
 * Rule = ttmi_beam_step_ctx's rule with these changes and no others:
 *  - Per live slot w and source j, lpx_j(w, k) = x_j[w][k] - L_j(w) in f32.  norm 0: L_j = 0 (the row holds log-probabilities; no pass is
 *    made over it).  norm 1: L_j = the row's log-sum-exp over all V entries, in one f32 pass exactly as the main row's.  norm 2: the
 *    log-sum-exp over all entries but the blank (the internal LM's renormalisation).  A row without a finite L_j has lpx_j = NaN throughout.
 *  - e(w, k) = sym_bonus + ext_0_w * (double)lpx_0(w, k) + ext_1_w * (double)lpx_1(w, k), accumulated in f64 in that order, every product
 *    and sum rounded on its own, absent sources skipped.
 *  - The extension of i by k carries fuse' = fuse_i + e(i, k), state and bias' as before, key = score + (bias' + fuse').  The blank extension
 *    of i carries fuse_i, key = score + (bias_i + fuse_i): the sources never touch it.
 *  - A symbol candidate whose e is not finite (NaN, +-inf) takes no slot.  A NaN key counts as -inf, as before.
 *  - A merged candidate takes i's state, bias and fuse (i's own stored values); which side's details it takes is decided by the two scores.
 *  - A finished utterance copies fuse through; an empty new slot gets fuse 0.
 * score_out stays the model's log-probability; bias_out is ttmi_beam_step_ctx's (the same f32 weights summed in the same order).  With both
 * sources absent and sym_bonus = 0 every output ttmi_beam_step_ctx also has is bit-identical to its, and fuse_out is 0 where fuse_in is.
 * The kernel reads a source row only for a live slot of an unfinished utterance.
 * rc < 0 with a ttmi_last_error text before any launch on anything ttmi_beam_step_ctx refuses, a null fuse buffer, fuse_out == fuse_in, a
 * non-finite sym_bonus, and per present source: a dtype outside 0..1, a norm outside 0..2, a non-finite weight, ext_j_ld < V, rows that
 * overlap an output buffer (the new beam's arrays, parent, fresh, state_out, bias_out, fuse_out, ws). */
size_t ttmi_beam_fuse_ws_bytes(int B, int W, int V);
int ttmi_beam_step_fuse(const void* logits, int dtype, long ld, int B, int W, int V, int blank, const int* t, const int* T_len,
                        const double* score_in, const int* len_in, const long* hist_in, const int* frames_in, const float* tok_lp_in,
                        double* score_out, int* len_out, long* hist_out, int* frames_out, float* tok_lp_out, long ld_hist, long ld_det,
                        int* parent, int* fresh, int S, int A, const int* arc_off, const int* arc_sym, const int* arc_next, const float* arc_w,
                        const int* fail, const float* fail_w, const int* state_in, const double* bias_in, int* state_out, double* bias_out,
                        void* ws, const double* fuse_in, double* fuse_out, double sym_bonus, const void* ext_0, int ext_0_dtype, long ext_0_ld,
                        double ext_0_w, int ext_0_norm, const void* ext_1, int ext_1_dtype, long ext_1_ld, double ext_1_w, int ext_1_norm,
                        void* stream);
/* The stable prefix of a beam: what a search that is still running (ttmi.beam.BeamSearch, the streaming recogniser) may show or act on.
 * In: one beam as ttmi_beam_step leaves it: score f64 [B, W], len i32 [B, W], hist i64 [B, W, ld_hist] with column 0 the start symbol.
 * Out: stable i32 [B].  A slot is live iff its score is > -inf (NaN and -inf are empty, the beam step's rule).  stable[b] = the largest
 * n >= 0 such that every live slot w has len[b][w] >= n and hist[b][w][1 + i] == hist[b][w0][1 + i] for all i < n, w0 the first live slot;
 * 0 without a live slot.  len is read clamped to [0, ld_hist - 1]: no index leaves a row whatever len holds.
 * Why the prefix is permanent: every slot of a new beam continues a slot of the old one (its parent's tokens, or those and one symbol more),
 * and a merge joins two candidates that spell the same tokens.  So what all live slots share, all their descendants share: the count of an
 * utterance never decreases from frame to frame, and the tokens it covers are those of every final hypothesis.
 * One wave per utterance: lanes across token positions, a loop over the slots, a wave-wide minimum of the first mismatch.  Ordinary vector
 * loads and one vector store of the result; no allocation, no host synchronisation, no memset node, no atomics: capturable in a HIP graph,
 * and two runs give the same bits.
 * rc < 0 with a ttmi_last_error text, before any launch, on a null pointer, W outside [1, 32], ld_hist < 1 or B < 0.  B = 0 succeeds and
 * does nothing. */
int ttmi_beam_stable_prefix(const double* score, const int* len, const long* hist, long ld_hist, int B, int W, int* stable, void* stream);

/* ---- error counting (ttmi.metrics: evaluation, and the per-hypothesis error counts of minimum word error rate training).
 * ttmi_edit_distance: token edit distance of P (hypothesis, transcript) pairs with its substitution / deletion / insertion counts.  One wave
 * per pair; it allocates nothing, does not synchronise with the host, uses no floating point and no atomics (two runs give the same bits).
 * In: hyp i32 [P, ld_hyp], hyp_len i32 [P]; ref i32 [n_ref, ld_ref], ref_len i32 [n_ref]; ref_index i32 [P] or NULL.  Pair p compares
 * hyp[p, :hyp_len[p]] with ref[r, :ref_len[r]], r = ref_index ? ref_index[p] : p (the N hypotheses of an utterance share one transcript
 * row).  Tokens are compared by equality only: any int32 value is a token.
 * Out: out i32 [P, 4] = (distance, substitutions, deletions, insertions); a deletion is a ref token without a hyp counterpart, an insertion a
 * hyp token without a ref counterpart, so distance = s + d + i and hyp_len = ref_len - d + i.
 * Limits: 0 <= max_hyp, max_ref <= 1024 (the lattice's own limit) and max_hyp <= ld_hyp, max_ref <= ld_ref; P >= 0, n_ref >= 0; no null
 * pointer (ref_index excepted) - else rc < 0 with a ttmi_last_error text, before any launch.  P = 0 succeeds and does nothing.
 * A pair whose hyp_len is outside [0, max_hyp], whose ref_index (or p, without one) is outside [0, n_ref) or whose ref_len is outside
 * [0, max_ref] is out of contract: it reads no token and writes (-1, -1, -1, -1); its neighbours are unaffected.
 * Rule: among all alignments the one that minimises (distance, substitutions, deletions, insertions) LEXICOGRAPHICALLY - the counts are
 * unique.  Equivalently the shortest path through the alignment grid with the integer edge costs
 *     match 0,  substitution (1 << 48) + (1 << 32),  deletion (1 << 48) + (1 << 16),  insertion (1 << 48) + 1
 * in int64; the four fields are read back from the path cost (bits 48.., 32..47, 16..31, 0..15: every field of a path is <= 2048). */
int ttmi_edit_distance(const int* hyp, long ld_hyp, const int* hyp_len, const int* ref, long ld_ref, const int* ref_len,
                       const int* ref_index /* nullable */, int P, int n_ref, int max_hyp, int max_ref, int* out /* [P, 4] */, void* stream);

/* ---- feature front-end on the GPU: replaces the data loader's per-utterance numpy code.
 * ttmi_logmel: get_feature / get_feature2 (tt/utils.py:182-207: librosa.feature.melspectrogram(y, sr, n_fft=512, hop_length=160, n_mels), then
 * log) for a batch.  wave i16 [B, pitch >= nmax] zero padded, n_samples i32 [B] (device) -> out f32 [B, Fmax, n_mels], Fmax = 1 + nmax / hop,
 * frames beyond 1 + n_b / hop zero.  The STFT is a GEMM with `dft` [2*(n_fft/2+1), n_fft] (rows 2k / 2k+1 = w[n] cos(2 pi k n / n_fft) /
 * -w[n] sin(...), analysis window w folded in), the filterbank a GEMM with mel_w [n_mels, n_fft/2+1]; log_mode 0 = np.ma.log(..).filled(0),
 * 1 = log10 with zeros -> float64 eps, 2 = none.  ws: ttmi_logmel_ws_floats floats, 256-byte aligned.
 * ttmi_stack_subsample: concat_frame + subsampling + Dataset.pad (tt/utils.py:120-151, tt/dataset.py:40-57) in one pass: feat f32 [B, Tin, F],
 * n_frames i32 [B] (device, nullable) -> out f32 [B, Tout, F*(1+left+right)], rows >= ceil(n_b / subsample) zero; out_lens nullable.
 * ttmi_spec_mask: frequency_mask_augment + time_mask_augment (tt/utils.py:297-329, train.py:41-44) in place on x f32 [B, T, F]; the (start,
 * width) pairs are HOST arrays (<= 32 per axis), drawn by the caller with the reference's RNG protocol. */
size_t ttmi_logmel_ws_floats(int B, int nmax, int n_fft, int hop);
int ttmi_logmel(const short* wave, long pitch, const int* n_samples, int B, int nmax, int n_fft, int hop, int n_mels, const float* dft,
                const float* mel_w, int log_mode, float* ws, float* out, void* stream);
int ttmi_stack_subsample(const float* feat, const int* n_frames, int B, int Tin, int F, int left, int right, int subsample, int Tout,
                         float* out, int* out_lens, void* stream);
int ttmi_spec_mask(float* x, int B, int T, int F, const int* time_spans, int n_time, const int* freq_spans, int n_freq, void* stream);

/* ---- training-step tail on flat f32 buffers: clip_grad_norm_ + optimizer.step (train.py:62-65, tt/optim.py:57-73)
 * normsq: device scalar holding sum(g^2) over ALL gradients (ttmi_sumsq accumulates into it); NULL = no clipping and no drop.
 * The effective gradient is g * grad_scale (1/world_size after a SUM all-reduce) clipped to max_norm (max_norm <= 0: not clipped).
 * A step whose *normsq is inf / NaN is DROPPED (parameters and state untouched) whatever max_norm is: the exp-domain loss form fails with
 * NaN costs and gradients by construction, and such a step must not reach the weights.
 * hyper (device float[3], nullable): the values that change between steps, read by the kernels at RUN time so that a step captured into a
 * HIP graph follows them - hyper[0] = learning rate (replaces `lr`: tt/optim.py:30-33 decay_lr, train.py:257), hyper[1] = optimiser steps
 * TAKEN, hyper[2] = steps DROPPED; every *_step call with hyper != NULL first advances hyper[1] by one on the device - or, when *normsq is
 * not finite, hyper[2]: a dropped step consumes no bias-correction step (Adam's corrections 1 - beta^hyper[1] replace the host's `step`). */
int ttmi_sumsq(const float* x, long n, float* out, void* stream);
int ttmi_sgd_step(float* p, const float* g, float* mom, long n, float lr, float momentum, float weight_decay, int nesterov,
                  float max_norm, const float* normsq, float grad_scale, float* hyper, void* stream);
int ttmi_adam_step(float* p, const float* g, float* m, float* v, long n, float lr, float beta1, float beta2, float eps,
                   float weight_decay, int step, float max_norm, const float* normsq, float grad_scale, float* hyper, void* stream);
/* torch.optim.Adadelta(lr, rho, eps, weight_decay), the third type of tt/optim.py:74-81 */
int ttmi_adadelta_step(float* p, const float* g, float* square_avg, float* acc_delta, long n, float lr, float rho, float eps,
                       float weight_decay, float max_norm, const float* normsq, float grad_scale, float* hyper, void* stream);

/* Mark a stream that is itself forked from the caller's main stream (the label encoder's side stream, tt/model.py _encode): calls on it never
 * fork onto the library's own side streams inside a stream capture (no reference counterpart; ttmi_set_option(18, 1) lets the capturing stream
 * itself fork as in eager mode). */
int ttmi_stream_set_nofork(void* stream, int on);

/* Device word (nullable) mixed into every dropout seed when a kernel starts.  Seeds are drawn on the host per sub-layer call; in a step that
 * is captured as a HIP graph they are baked into the kernel arguments, so the caller bumps this word on the device before each replay
 * (ttmi.train.GraphedStep) and every step still draws fresh masks.  Forward and backward of one step must see the same value. */
int ttmi_set_dropout_salt(const unsigned* salt);

/* ---- bring-up / measurement helpers ------------------------------------------------------------------------------
 * generic MFMA GEMM (every layout / dtype / epilogue; flags = GemmFlags of csrc/gemm.h) and the two throughput
 * kernels; HIP-event probes recorded on the launch stream at five points (0 = joint vocabulary projection, 1 = ttmi_rnnt_loss_fwd's
 * kernels, 2 = ttmi_rnnt_loss_bwd's kernel, 3 = the fused attention backward kernel of a layer with L >= 256, 4 = a grouped weight-gradient launch of
 * ttmi_wgrad_group that fills at least half the chip): ttmi_probe_arm(i), 0 <= i < 64, makes the NEXT launch at every point record into its event
 * pair i; ttmi_probe_point_read_ms(point, i) waits for that pair and returns its duration in ms (< 0: never fired);
 * ttmi_probe_read_ms(i) = point 0. */
int ttmi_gemm(const void* A, const void* B, void* C, const float* bias, const float* aux, int a_dtype, int b_dtype,
              int c_dtype, int M, int N, int K, long lda, long ldb, long ldc, int nz1, int nz2, long sA1, long sA2,
              long sB1, long sB2, long sC1, long sC2, float alpha, float beta, int flags, int splitk, void* stream);
int ttmi_gemm_nt_bf16(const void* A, const void* B, void* C, int c_dtype, const float* bias, int M, int N, int K, long lda,
                      long ldb, long ldc, void* stream);
/* bring-up entry of the two-term weight form (option 13): C = epi(A.(B + B_lo)^T), B_lo [N, K] bf16 with B's pitch, in ONE launch - the persistent
 * kernels walk A's K-tiles a second time against B_lo, the 128x128 kernel takes (A, B_lo) as its second operand pair */
int ttmi_gemm_nt_bf16_two_term(const void* A, const void* B, const void* B_lo, void* C, int c_dtype, const float* bias, int relu, int M, int N, int K,
                               long lda, long ldb, long ldc, void* stream);
/* ... with the second walk limited to A's first k_lo columns (0 = all K): C = act(A.B^T + A[:, :k_lo].B_lo[:, :k_lo]^T + bias) - the layout of the
 * bf16x3 products, A = [hi | lo], B = [hi | hi], B_lo = lo (k_lo = K / 2) */
int ttmi_gemm_nt_bf16_two_term_klo(const void* A, const void* B, const void* B_lo, void* C, int c_dtype, const float* bias, int relu, int M, int N, int K,
                                   int k_lo, long lda, long ldb, long ldc, void* stream);
/* bring-up entry of the "exp store" epilogue of the persistent 256x256 kernel: C = bf16(exp(A.B^T + bias - shift)) with zeros in columns [N, ldc),
 * rowsum [nparts, M] = per-row partial sums (nparts >= 4 * ceil(N / 256); the entries of a row add up to its sum of exponentials) */
int ttmi_gemm_nt_bf16_exp(const void* A, const void* B, void* C, const float* bias, float* rowsum, int nparts, const float* shift /* device, nullable */, int M, int N, int K,
                          long lda, long ldb, long ldc, void* stream);
/* bring-up entry of the "row factor" epilogue of the persistent 256x256 kernel (the joint's dgrad in the exp-domain loss form, the adjoint of
 * tt/model.py:34-38 with the loss gradient kept factored): C = bf16((A.B^T) * (1 - mask^2) * rowscale[m]) and, in place, mask <- rowscale[m] * mask
 * (mask bf16 [M, ldc], the layout of C; rowscale f32 [M]) */
int ttmi_gemm_nt_bf16_rowscale(const void* A, const void* B, void* C, void* mask, const float* rowscale, int M, int N, int K, long lda, long ldb, long ldc,
                               void* stream);
int ttmi_gemm_tn_bf16(const void* A, const void* B, float* C, int M, int N, int K, long lda, long ldb, long ldc, int accumulate,
                      float* colsum_a /* nullable: colsum_a[m] += sum_k A[k][m] */, void* stream);
/* bring-up entry of the weighted column sums (persistent 256x256 TN kernel only: K >= 32768, M >= 1024, N % 256 == 0, N >= 1024):
 * C += A^T B and colsum_a[m] += sum_k colsum_w[k] A[k][m] (colsum_w bf16 [K], 16-byte aligned) */
int ttmi_gemm_tn_bf16_wsum(const void* A, const void* B, float* C, int M, int N, int K, long lda, long ldb, long ldc, float* colsum_a,
                           const void* colsum_w, void* stream);
/* bf16 shadows of GEMM weights.  Every forward call otherwise converts its f32 master weights to bf16 (plain + transposed copies: 118
 * launches per step at C2 for weights that change once per optimiser step).  A training loop registers, per weight w [R, C], a plain bf16
 * copy w16 [R, C] and a transposed one wT16 [C, ldT] (ldT >= R, columns [R, ldT) zero) and rebuilds ALL of them with one launch after each
 * update (ttmi_weight_shadow_refresh: `table` = device array of n rows of 8 longs (w, R, C, wT16, ldT, w16, first 32x32 tile, tiles along C),
 * sorted by first tile; total_tiles = their sum).  The sub-layer calls look a shadow up by the f32 pointer and use it when its geometry
 * matches, else convert as before.  The caller owns the memory and the freshness (ttmi.train.FlatModel). */
int ttmi_weight_shadow_register(const float* w, int R, int C, const void* w16, const void* wT16, long ldT);
int ttmi_weight_shadow_clear(const float* w /* NULL = all */);
int ttmi_weight_shadow_refresh(const long* table, int n, long total_tiles, void* stream);
/* round 6: the second term of a shadowed weight's bf16 split, w16lo = bf16(w - float(w16)) (the operand of ttmi_set_option(13, ...)), kept with the shadows: one
 * buffer of twice the plain copies' size, w16lo at w16 + lo_delta elements; ttmi_weight_shadow_refresh_lo rebuilds all three copies in its one launch.  Without
 * it every forward call that takes the second term forms it itself (one small launch per GEMM). */
int ttmi_weight_shadow_register_lo(const float* w, const void* w16lo);
int ttmi_weight_shadow_refresh_lo(const long* table, int n, long total_tiles, long lo_delta, void* stream);

/* data-parallel runs (train.py:55-56,214-219 replaced by one process per GPU + RCCL): the gradient all-reduce kernels run beside the
 * backward pass; the encoder-sized persistent GEMMs launched on `stream` (and on the library's fork streams serving it) leave n CUs to
 * them.  Per-stream state read at launch time; 0 = whole chip (default). */
int ttmi_stream_reserve_cus(void* stream, int n);
/* process-wide A/B switches for MEASUREMENTS ONLY (not thread-safe against concurrent launches, no product path depends on them): key 0: 1 = no fused attention kernels; 1: throughput-GEMM generation (csrc/gemm_fast.hip; 5 = nothing persistent: every eligible NT problem on 64x64 tiles; 14 / 15 = streaming output stores off / on; 16 + n = the 64x64-tile bf16 NT kernel from n of its tiles on, 16 = never, default 48);
 * 2: flash-kernel timing bits; 3: 0 = no side-stream wgrad fork; 4: split-K workgroup target; 5: 1 = position-term slab by batched GEMM;
 * 6: process-wide default of ttmi_stream_reserve_cus for streams that never set one;
 * 7: exact-f32 products with at most n rows use the skinny 32x32 split-reduction kernel (default 128, 0 = never: greedy decode A/B);
 * 8: 0 = the fused attention kernels read the position term from a [B,H,L,L+1] bf16 slab (round-1 design) instead of forming it themselves;
 * 9: 1 = one-wave lattice kernel (round 2) instead of the workgroup-per-utterance one; 10: batch slices of the attention backward; 11: 1 = dq / dE /
 * dc by the round-2 GEMM launches instead of attn_dqde_kernel; 12: workgroups of the grid-stride LayerNorm backward kernels; 13 (default 2 since round 6): 1 = the four
 * forward GEMMs of an encoder layer (qkv_net, o_net, CoreNet.0, CoreNet.3) take the second term of their weight's bf16 split as a second K range, one launch each; 2 = o_net and
 * CoreNet.3 only, in stacks of at least 4096 rows (the audio encoder; the label states' value has its own pass); + 4 = all four in stacks of fewer than 4096 rows (the label encoder); 0 = off (2: +0.4 ms per C2 step - with the label encoder's value pass
 * of tt.model the timed mode's batch-mean loss stays within 8.1e-5 of the fp32 mode over 56 training states, profiles/r06_loss_error_batch_mean_fixed.log); 14: 0 = the tiled attention
 * forward kernel instead of the one-workgroup-per-head one; 15: 1 = the round-3 attention backward kernel instead of flash_bwd_rel2_kernel;
 * 16: 1 = the position-table gradients go through dE / dc and a relpos_scatter launch (round 3) instead of straight out of attn_dqde_kernel;
 * 17: exact-f32 NT products: 0 = the kernels of csrc/gemm.hip only (round 1), 1 = default rule (persistent 256x128 kernel with f32 operands from 512 of its tiles on,
 * 64x64 tiles from 72 of those on), 2 / 3 = the 64x64-tile / the persistent kernel wherever it can run; 18: 1 = fork inside a stream capture;
 * 19: 0 = the joint's input layer (bf16 mode) without the second bf16 term of the label-encoder states (round 6: that rounding is one pattern in all T lattice rows of a label
 * position and was the joint's whole share of the batch-mean loss error; A/B);
 * 20: 0 = grouped weight gradients never cut an XCD's surplus tiles into K-pieces (default 1: under a CU reservation - ttmi_stream_reserve_cus - 256 tiles on 224 ... 248
 * workgroups end with one atomically added piece per workgroup instead of a second round; without a reservation the launches stay free of atomics either way);
 * 21: 0 = the joint's sums over frames (dPD) by f32 atomics as in rounds 1 - 5 (default 1: partial rows + an ordered second pass - the same bits in every run, same time);
 * 22: 0 = bf16x3 weight gradients as three accumulating launches (round 5) instead of one launch over the plane pairs + a fold;
 * 23: ttmi_rnnt_align / ttmi_mono_align / ttmi_ctc_align bits: 1 = decision words in the caller's workspace whatever the shape, 2 = forward walk only, no backtrace (frames of real labels are not written) */
int ttmi_set_option(int key, int value);
int ttmi_dropout_apply(const float* in, long n, float p, unsigned seed, float* out, void* stream);
int ttmi_probe_arm(int slot);
float ttmi_probe_read_ms(int slot);
float ttmi_probe_point_read_ms(int point, int slot);

#ifdef __cplusplus
}
#endif
#endif
