// Token edit distance with unique substitution / deletion / insertion counts, for gfx950 (error counting for evaluation and the W_i of
// minimum word error rate training; the reference counts errors on the host with the `editdistance` package).
//
//   edit_distance_kernel<C>   latency-bound dynamic programme, ONE WAVE PER PAIR, four waves per workgroup (the waves of a workgroup share
//                             nothing: no LDS, no barrier).  Lane l owns the C contiguous ref columns l*C + 1 .. l*C + C (C = 1, 2, 4, 8, 16:
//                             64 C >= max_ref <= 1024); the loop runs over the hyp rows.  The previous row lives in REGISTERS (C int64 per
//                             lane, fully unrolled; DESIGN.md section 4o has the compiler's resource report).  Path costs are int64 with the
//                             four fields packed as the header states (include/ttmi.h, ttmi_edit_distance), so ONE integer minimum takes the
//                             lexicographic minimum of (distance, substitutions, deletions, insertions).
//                             A row:  t_k = min(D[i-1][k] + c_ins, D[i-1][k-1] + c_diag)   (the moves that consume hyp token i)
//                                     D[i][j] = j c_del + min over k <= j of (t_k - k c_del) (then any number of deletions along the row)
//                             i.e. a local prefix minimum over the lane's columns, one exclusive 64-lane min-scan of the lanes' totals
//                             (__shfl_up, six steps) and a carry.  The fields of t_k - k c_del may borrow; the comparison of those integers is
//                             still the comparison of the path costs (the same j c_del is added to both sides of every comparison made for
//                             column j).  Largest magnitude: 2048 edges of < 2^49 each, < 2^60.
//                             No floating point, no atomics: two runs give the same bits.
#include "common.h"

namespace {

constexpr int ED_WAVES = 4;
constexpr long long ED_UNIT = 1LL << 48;
constexpr long long ED_SUB = ED_UNIT + (1LL << 32);
constexpr long long ED_DEL = ED_UNIT + (1LL << 16);
constexpr long long ED_INS = ED_UNIT + 1LL;
constexpr long long ED_INF = 0x7fffffffffffffffLL;

__device__ __forceinline__ long long min64(long long a, long long b) { return a < b ? a : b; }

template <int C>
__global__ __launch_bounds__(ED_WAVES * 64) void edit_distance_kernel(
    const int* __restrict__ hyp, long ld_hyp, const int* __restrict__ hyp_len, const int* __restrict__ ref, long ld_ref,
    const int* __restrict__ ref_len, const int* __restrict__ ref_index, int P, int n_ref, int max_hyp, int max_ref, int* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long p = (long)blockIdx.x * ED_WAVES + (threadIdx.x >> 6);
    if (p >= P) return;                                   // (wave-uniform, as everything below that branches)
    const long r = ref_index ? (long)ref_index[p] : p;
    const int m = hyp_len[p];
    const bool ref_ok = r >= 0 && r < n_ref;
    const int n = ref_ok ? ref_len[r] : -1;
    if (!ref_ok || m < 0 || m > max_hyp || n < 0 || n > max_ref) {      // out of contract: no token is read
        if (lane < 4) out[p * 4 + lane] = -1;
        return;
    }
    const int* h = hyp + p * ld_hyp;
    const int* y = ref + r * ld_ref;
    const int j0 = lane * C + 1;                          // this lane's first column (column 0 = the empty ref prefix, held in closed form)
    int tok[C];
    long long prev[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int j = j0 + c;
        tok[c] = j <= n ? y[j - 1] : 0;                   // columns past the transcript: computed, never read by a column <= n
        prev[c] = (long long)j * ED_DEL;                  // row 0: j deletions
    }
    int hv = 0;
    for (int i = 1; i <= m; ++i) {
        if (((i - 1) & 63) == 0) hv = (i - 1 + lane < m) ? h[i - 1 + lane] : 0;      // the next 64 hyp tokens, one per lane
        const int hi = __shfl(hv, (i - 1) & 63, 64);
        long long left = __shfl_up(prev[C - 1], 1, 64);   // D[i-1][j0 - 1]: the last column of the lane before
        if (lane == 0) left = (long long)(i - 1) * ED_INS;
        long long run = ED_INF;
        long long loc[C];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const long long t = min64(prev[c] + ED_INS, left + (tok[c] == hi ? 0LL : ED_SUB));
            left = prev[c];
            run = min64(run, t - (long long)(j0 + c) * ED_DEL);
            loc[c] = run;
        }
        long long scan = run;                             // inclusive min-scan of the lanes' totals
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const long long up = __shfl_up(scan, o, 64);
            if (lane >= o) scan = min64(scan, up);
        }
        long long carry = __shfl_up(scan, 1, 64);         // what the lanes to the left hand on
        const long long col0 = (long long)i * ED_INS;     // t_0 - 0 c_del: the empty ref prefix after i insertions
        carry = lane == 0 ? col0 : min64(carry, col0);
#pragma unroll
        for (int c = 0; c < C; ++c) prev[c] = (long long)(j0 + c) * ED_DEL + min64(carry, loc[c]);
    }
    // D[m][n]: column n belongs to lane (n - 1) / C (n = 0: i insertions)
    long long cost = (long long)m * ED_INS;
#pragma unroll
    for (int c = 0; c < C; ++c)
        if (j0 + c == n) cost = prev[c];
    const int owner = n > 0 ? (n - 1) / C : 0;
    if (lane == owner) {
        out[p * 4 + 0] = (int)(cost >> 48);               // every field of a finished path is in [0, 2048]: nothing borrows here
        out[p * 4 + 1] = (int)((cost >> 32) & 0xffff);
        out[p * 4 + 2] = (int)((cost >> 16) & 0xffff);
        out[p * 4 + 3] = (int)(cost & 0xffff);
    }
}

template <int C>
void launch(hipStream_t st, const int* hyp, long ld_hyp, const int* hyp_len, const int* ref, long ld_ref, const int* ref_len,
            const int* ref_index, int P, int n_ref, int max_hyp, int max_ref, int* out) {
    hipLaunchKernelGGL(edit_distance_kernel<C>, dim3(cdiv(P, ED_WAVES)), dim3(ED_WAVES * 64), 0, st, hyp, ld_hyp, hyp_len, ref, ld_ref, ref_len,
                       ref_index, P, n_ref, max_hyp, max_ref, out);
}

}  // namespace

extern "C" {

int ttmi_edit_distance(const int* hyp, long ld_hyp, const int* hyp_len, const int* ref, long ld_ref, const int* ref_len, const int* ref_index,
                       int P, int n_ref, int max_hyp, int max_ref, int* out, void* stream) {
    TTMI_REQUIRE(P >= 0 && n_ref >= 0, "edit_distance: bad counts P=%d n_ref=%d", P, n_ref);
    TTMI_REQUIRE(max_hyp >= 0 && max_hyp <= 1024 && max_ref >= 0 && max_ref <= 1024,
                 "edit_distance: max_hyp=%d / max_ref=%d outside [0, 1024]", max_hyp, max_ref);
    TTMI_REQUIRE(max_hyp <= ld_hyp && max_ref <= ld_ref, "edit_distance: bad pitch (max_hyp=%d ld_hyp=%ld, max_ref=%d ld_ref=%ld)", max_hyp,
                 ld_hyp, max_ref, ld_ref);
    if (P == 0) return TTMI_OK;
    TTMI_REQUIRE((hyp || max_hyp == 0) && hyp_len && (ref || max_ref == 0 || n_ref == 0) && (ref_len || n_ref == 0) && out,
                 "edit_distance: null pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
#define TTMI_ED_LAUNCH(C) launch<C>(st, hyp, ld_hyp, hyp_len, ref, ld_ref, ref_len, ref_index, P, n_ref, max_hyp, max_ref, out)
    if (max_ref <= 64) TTMI_ED_LAUNCH(1);
    else if (max_ref <= 128) TTMI_ED_LAUNCH(2);
    else if (max_ref <= 256) TTMI_ED_LAUNCH(4);
    else if (max_ref <= 512) TTMI_ED_LAUNCH(8);
    else TTMI_ED_LAUNCH(16);
#undef TTMI_ED_LAUNCH
    TTMI_LAUNCH_CHECK("edit_distance_kernel");
    return TTMI_OK;
}

}  // extern "C"
