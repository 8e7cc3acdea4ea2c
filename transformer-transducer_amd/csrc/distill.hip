// Transducer knowledge distillation on collapsed lattice posteriors (Panchapagesan et al., ICASSP 2021) for gfx950: every lattice node's
// distribution over V outputs is collapsed to three classes - blank, the next label y_{u+1}, everything else - and the student is trained
// with the KL divergence from the teacher's three to its own three (include/ttmi.h has the arithmetic).  No reference counterpart.
//
//   kd_row_kernel    HBM-bound: one wave per (b,t,u) row of V logits, lattice.h's row_lse walk - taken over the
//                    columns OUTSIDE {blank, y} only, so the "other" mass is a log-sum-exp of its own and never 1 - p_b - p_y; the row's lse is
//                    that sum joined with the two columns left out (three terms, lane 0).  TEACHER = false writes the collapsed posteriors,
//                    TEACHER = true reads the teacher's and writes the row's record (lse, c_o, P^T_b, P^T_y) and its cost.
//   kd_sum_kernel    one workgroup per utterance adds its nodes' row costs in fp64, in an order fixed by the shape alone.
//   kd_grad_kernel   HBM-bound: one wave per row reads the logits once and writes the gradient once (in place allowed), or, ACC = true, adds it
//                    to the gradient already there (widened to f32, rounded once) and touches nothing else.
#include "common.h"
#include "lattice.h"

namespace {

using namespace ttmi_lattice;

constexpr int KD_WAVES = 4;
constexpr int KD_SUM_THREADS = 1024;      // (a C2 utterance has 25 500 nodes: 25 loads per thread, then ten tree steps)

struct KdWs {
    float4* rec;                           // [B, T, U1] (lse, c_o, P^T_b, P^T_y)
    float* cost;                           // [B, T, U1]
};
KdWs kd_carve(void* ws, int B, int T, int U1) {
    KdWs w;
    w.rec = static_cast<float4*>(ws);      // (workspace must be 16-byte aligned)
    w.cost = reinterpret_cast<float*>(w.rec + (long)B * T * U1);
    return w;
}

__device__ __forceinline__ float kd_floor(float x) { return x < NEG ? NEG : x; }      // (a NaN stays a NaN)

// ------------------------------------------------------------------ collapse (teacher) / collapse + KL (student)
template <typename TL, bool TEACHER>
__global__ __launch_bounds__(KD_WAVES * 64) void kd_row_kernel(
    const TL* __restrict__ logits, long ldv, const int* __restrict__ labels, const int* __restrict__ act_lens,
    const int* __restrict__ label_lens, int B, int T, int U1, int V, int blank, int vec_ok, const float* __restrict__ teacher,
    float* __restrict__ post, float4* __restrict__ rec, float* __restrict__ cost) {
    constexpr int NV = Vec16<TL>::NV;
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * KD_WAVES + (threadIdx.x >> 6);
    if (row >= (long)B * T * U1) return;
    const LatticeRow p = lattice_row(row, T, U1, act_lens, label_lens);
    const int b = p.b, u = p.u, Ub = p.Ub;
    if (!p.inside()) {
        // the posteriors are a tensor the caller keeps: exact zeros outside the ragged lattice; the student's records there are never read
        if constexpr (!TEACHER)
            if (lane < 3) post[row * 3 + lane] = 0.f;
        return;
    }
    int yv = -1;                           // the label class is empty at u == U_b and for a label equal to blank
    if (u < Ub) {
        yv = clampi(labels[(long)b * (U1 - 1) + u], 0, V - 1);
        if (yv == blank) yv = -1;
    }
    const TL* r = logits + row * ldv;
    // a column of {blank, y} enters as -inf: exp(-inf - mn) = 0 whatever the running maximum (which never falls below NEG)
    auto other = [&](float x, int v) -> float { return (v == blank || v == yv) ? -INFINITY : x; };
    float M, s;
    row_lse<TL>(r, V, vec_ok, lane, M, s, other, [&](Vec16<TL>& x, int v0) {
        // two columns of the row are left out: one range test per 16 bytes, and the per-element selects only in the vector that holds one
        if ((unsigned)(blank - v0) < (unsigned)NV || (unsigned)(yv - v0) < (unsigned)NV) {
#pragma unroll
            for (int k = 0; k < NV; ++k) x.f[k] = other(x.f[k], v0 + k);
        }
    });
    if (lane == 0) {
        const float lo_raw = M + __logf(s);                    // -inf when no other column carries mass (V = 2, or all of them -inf)
        const float zb = ldf<TL>(r + blank);
        const float zy = yv >= 0 ? ldf<TL>(r + yv) : -INFINITY;
        const float M3 = fmaxf(fmaxf(M, zb), zy);
        const float l = M3 + __logf(s * __expf(M - M3) + __expf(zb - M3) + __expf(zy - M3));
        const float lb = kd_floor(zb - l);
        const float ly = yv >= 0 ? kd_floor(zy - l) : NEG;
        const float lo = kd_floor(lo_raw - l);
        if constexpr (!TEACHER) {
            post[row * 3 + 0] = lb;
            post[row * 3 + 1] = ly;
            post[row * 3 + 2] = lo;
        } else {
            const float tb = teacher[row * 3 + 0], ty = teacher[row * 3 + 1], to = teacher[row * 3 + 2];
            const float pb = __expf(tb), po = __expf(to);
            const float py = yv >= 0 ? __expf(ty) : 0.f;       // an empty label class takes nothing from the teacher
            // a class the teacher gives no mass adds exactly 0 (not 0 * (NEG - ...)); a NaN entry fails `== 0` and stays a NaN
            float c = 0.f;
            c += pb == 0.f ? 0.f : pb * (tb - lb);
            c += py == 0.f ? 0.f : py * (ty - ly);
            c += po == 0.f ? 0.f : po * (to - lo);
            // c_o = P^T_o / P^S_o from the two log-probabilities; 0 when the class is empty on either side (the teacher's: the other columns
            // get s_k; the student's: every s_k there is 0 and the ratio must not turn it into a NaN)
            const float co = (to <= NEG || lo <= NEG) ? 0.f : __expf(to - lo);
            rec[row] = make_float4(l, co, pb, py);
            cost[row] = c;
        }
    }
}

// ------------------------------------------------------------------ per-utterance sum of the row costs
__global__ __launch_bounds__(KD_SUM_THREADS) void kd_sum_kernel(const float* __restrict__ cost, const int* __restrict__ act_lens,
                                                                const int* __restrict__ label_lens, int T, int U1,
                                                                float* __restrict__ costs) {
    __shared__ acc_t part[KD_SUM_THREADS];
    const int b = blockIdx.x;
    const int Tb = clampi(act_lens[b], 1, T), Ub = clampi(label_lens[b], 0, U1 - 1);
    const float* c = cost + (long)b * T * U1;
    const int n = Tb * U1;                 // rows of frames [0, T_b); the columns u > U_b among them are skipped
    acc_t a = 0.0;
    for (int i = threadIdx.x; i < n; i += KD_SUM_THREADS)
        if (i % U1 <= Ub) a += (acc_t)c[i];
    part[threadIdx.x] = a;
    __syncthreads();
    // a tree whose shape depends on nothing but the thread count: the same order in every run
    for (int w = KD_SUM_THREADS / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) costs[b] = (float)part[0];
}

// ------------------------------------------------------------------ gradient
template <typename TL, bool ACC>
__global__ __launch_bounds__(KD_WAVES * 64) void kd_grad_kernel(
    const TL* logits, long ldv, const int* __restrict__ labels, const int* __restrict__ act_lens, const int* __restrict__ label_lens,
    int B, int T, int U1, int V, int blank, int vec_ok, const float4* __restrict__ rec, const float* __restrict__ grad_out,
    int grad_out_stride, float scale, TL* grad, long ldg) {
    constexpr int NV = Vec16<TL>::NV;
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * KD_WAVES + (threadIdx.x >> 6);
    if (row >= (long)B * T * U1) return;
    const LatticeRow p = lattice_row(row, T, U1, act_lens, label_lens);
    const int b = p.b, u = p.u, Ub = p.Ub;
    const bool valid = p.inside();
    if (ACC && !valid) return;             // accumulate: nothing outside the lattice's rows is touched
    const TL* r = logits + row * ldv;
    TL* g = grad + row * ldg;
    float l = 0.f, ko = 0.f, pb = 0.f, py = 0.f, gs = 0.f;
    int yv = -1;
    if (valid) {
        const float4 q = rec[row];
        l = q.x;
        ko = 1.f - q.y;
        pb = q.z;
        py = q.w;
        gs = scale * grad_out[(long)b * grad_out_stride];
        if (u < Ub) {
            yv = clampi(labels[(long)b * (U1 - 1) + u], 0, V - 1);
            if (yv == blank) yv = -1;
        }
    }
    auto f = [&](float x, int v) -> float {
        const float e = __expf(x - l);
        const float d = (v == blank) ? e - pb : ((v == yv) ? e - py : e * ko);
        return valid ? gs * d : 0.f;
    };
    // f for a vector that holds neither the blank nor the label column (one range test per 16 bytes): the same arithmetic, no selects
    auto fo = [&](float x) -> float { return valid ? gs * (__expf(x - l) * ko) : 0.f; };
    auto special = [&](int v0) -> bool { return (unsigned)(blank - v0) < (unsigned)NV || (unsigned)(yv - v0) < (unsigned)NV; };
    if constexpr (ACC) {
        // the one read-modify-write walk, and the one that must leave the pad columns [V, ldg) alone: not a row_map
        const int head = row_head<TL>(r, V, vec_ok);
        const int nvec = (V - head) / NV;
        for (int i = lane; i < head; i += 64) stf<TL>(g + i, ldf<TL>(g + i) + f(ldf<TL>(r + i), i));
        for (int i = lane; i < nvec; i += 64) {
            Vec16<TL> x, a;
            const int v0 = head + i * NV;
            x.load(r + v0);
            a.load(g + v0);
            if (special(v0)) {
#pragma unroll
                for (int k = 0; k < NV; ++k) a.f[k] += f(x.f[k], v0 + k);
            } else {
#pragma unroll
                for (int k = 0; k < NV; ++k) a.f[k] += fo(x.f[k]);
            }
            a.store(g + v0);
        }
        for (int i = head + nvec * NV + lane; i < V; i += 64) stf<TL>(g + i, ldf<TL>(g + i) + f(ldf<TL>(r + i), i));
    } else {
        // in place: every lane overwrites only the elements it has read itself, and the row's record lives in the workspace
        row_map<TL>(r, g, V, ldg, vec_ok, lane, valid, f, [&](Vec16<TL>& x, int v0) {
            if (special(v0)) {
#pragma unroll
                for (int k = 0; k < NV; ++k) x.f[k] = f(x.f[k], v0 + k);
            } else {
#pragma unroll
                for (int k = 0; k < NV; ++k) x.f[k] = fo(x.f[k]);
            }
        });
    }
}

template <typename TL, bool TEACHER>
void kd_launch_rows(hipStream_t st, const void* logits, long ldv, const int* labels, const int* act_lens, const int* label_lens, int B, int T,
                    int U1, int V, int blank, const float* teacher, float* post, float4* rec, float* cost) {
    const long rows = (long)B * T * U1;
    const int vec_ok = rows_vec_ok(logits, sizeof(TL));
    hipLaunchKernelGGL((kd_row_kernel<TL, TEACHER>), dim3(cdiv(rows, KD_WAVES)), dim3(KD_WAVES * 64), 0, st, static_cast<const TL*>(logits), ldv,
                       labels, act_lens, label_lens, B, T, U1, V, blank, vec_ok, teacher, post, rec, cost);
}

template <typename TL, bool ACC>
void kd_launch_grad(hipStream_t st, const void* logits, long ldv, const int* labels, const int* act_lens, const int* label_lens, int B, int T,
                    int U1, int V, int blank, const float4* rec, const float* grad_out, int grad_out_stride, float scale, void* grad, long ldg) {
    const long rows = (long)B * T * U1;
    const int vec_ok = rows_vec_ok(logits, grad, ldv, ldg, sizeof(TL));
    hipLaunchKernelGGL((kd_grad_kernel<TL, ACC>), dim3(cdiv(rows, KD_WAVES)), dim3(KD_WAVES * 64), 0, st, static_cast<const TL*>(logits), ldv,
                       labels, act_lens, label_lens, B, T, U1, V, blank, vec_ok, rec, grad_out, grad_out_stride, scale, static_cast<TL*>(grad), ldg);
}

}  // namespace

extern "C" {

// bytes of caller-provided workspace shared by ttmi_kd_loss_fwd / _bwd (16-byte aligned): one 16-byte record and one f32 cost per row
size_t ttmi_kd_workspace_bytes(int B, int T, int U1) {
    if (B <= 0 || T <= 0 || U1 <= 0) return 0;
    return (sizeof(float4) + sizeof(float)) * (size_t)B * T * U1;
}

#define KD_CHECK_COMMON(name)                                                                                                        \
    TTMI_REQUIRE(B > 0 && T > 0 && U1 > 0, name ": bad shape B=%d T=%d U1=%d", B, T, U1);                                            \
    TTMI_REQUIRE(V >= 2, name ": V=%d < 2 (a blank and at least one label)", V);                                                     \
    TTMI_REQUIRE(ldv >= V && (dtype == 0 || dtype == 1), name ": bad pitch/dtype");                                                  \
    TTMI_REQUIRE(blank >= 0 && blank < V, name ": blank %d outside [0,%d)", blank, V);                                               \
    TTMI_REQUIRE((long)B * T * U1 <= 0x7fffffffL / 4, name ": B*T*U1 = %ld rows unsupported", (long)B * T * U1)

int ttmi_kd_collapse(const void* logits, int dtype, long ldv, const int* labels, const int* act_lens, const int* label_lens, int B, int T,
                     int U1, int V, int blank, float* post, void* stream) {
    TTMI_REQUIRE(logits && (labels || U1 == 1) && act_lens && label_lens && post, "kd_collapse: null pointer");
    KD_CHECK_COMMON("kd_collapse");
    hipStream_t st = static_cast<hipStream_t>(stream);
    by_dtype(dtype, [&](auto z) {
        kd_launch_rows<decltype(z), false>(st, logits, ldv, labels, act_lens, label_lens, B, T, U1, V, blank, nullptr, post, nullptr, nullptr);
    });
    TTMI_LAUNCH_CHECK("kd_row_kernel");
    return TTMI_OK;
}

int ttmi_kd_loss_fwd(const void* logits, int dtype, long ldv, const int* labels, const int* act_lens, const int* label_lens, int B, int T,
                     int U1, int V, int blank, const float* teacher, void* workspace, float* costs, void* stream) {
    TTMI_REQUIRE(logits && (labels || U1 == 1) && act_lens && label_lens && teacher && workspace && costs, "kd_loss_fwd: null pointer");
    KD_CHECK_COMMON("kd_loss_fwd");
    TTMI_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "kd_loss_fwd: workspace must be 16-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const KdWs w = kd_carve(workspace, B, T, U1);
    by_dtype(dtype, [&](auto z) {
        kd_launch_rows<decltype(z), true>(st, logits, ldv, labels, act_lens, label_lens, B, T, U1, V, blank, teacher, nullptr, w.rec, w.cost);
    });
    TTMI_LAUNCH_CHECK("kd_row_kernel");
    hipLaunchKernelGGL(kd_sum_kernel, dim3(B), dim3(KD_SUM_THREADS), 0, st, w.cost, act_lens, label_lens, T, U1, costs);
    TTMI_LAUNCH_CHECK("kd_sum_kernel");
    return TTMI_OK;
}

int ttmi_kd_loss_bwd(const void* logits, int dtype, long ldv, const int* labels, const int* act_lens, const int* label_lens, int B, int T,
                     int U1, int V, int blank, const void* workspace, const float* grad_out, int grad_out_stride, float scale, void* grad,
                     long ldg, int accumulate, void* stream) {
    TTMI_REQUIRE(logits && (labels || U1 == 1) && act_lens && label_lens && workspace && grad_out && grad, "kd_loss_bwd: null pointer");
    KD_CHECK_COMMON("kd_loss_bwd");
    TTMI_REQUIRE(ldg >= V, "kd_loss_bwd: bad gradient pitch");
    TTMI_REQUIRE(accumulate == 0 || accumulate == 1, "kd_loss_bwd: accumulate must be 0 or 1, got %d", accumulate);
    TTMI_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "kd_loss_bwd: workspace must be 16-byte aligned");
    TTMI_REQUIRE(logits != static_cast<const void*>(grad) || ldg == ldv, "kd_loss_bwd: in-place needs ldg == ldv");
    TTMI_REQUIRE(logits != static_cast<const void*>(grad) || !accumulate, "kd_loss_bwd: accumulate = 1 cannot add to the logits themselves");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const KdWs w = kd_carve(const_cast<void*>(workspace), B, T, U1);
    by_dtype(dtype, [&](auto z) {
        using TL = decltype(z);
        if (accumulate)
            kd_launch_grad<TL, true>(st, logits, ldv, labels, act_lens, label_lens, B, T, U1, V, blank, w.rec, grad_out, grad_out_stride, scale, grad, ldg);
        else
            kd_launch_grad<TL, false>(st, logits, ldv, labels, act_lens, label_lens, B, T, U1, V, blank, w.rec, grad_out, grad_out_stride, scale, grad, ldg);
    });
    TTMI_LAUNCH_CHECK("kd_grad_kernel");
    return TTMI_OK;
}

}  // extern "C"
