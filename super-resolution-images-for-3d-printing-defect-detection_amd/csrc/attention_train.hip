// attention_train.hip -- SelfAttention (ESRGAN_model.py:57-65) for TRAINING without the N x N attention map: the fp32 streaming forward
// that also keeps lse_i = m_i + log(l_i) per query, and a streamed backward that recomputes P_ij = exp(s_ij - lse_i) tile by tile.
// d_qk = 8, d_v = 32, no 1/sqrt(d) scale, everything fp32 on v_mfma_f32_32x32x2_f32.  With D_i = <dO_i, o_i>:
//   dV_j = sum_i P_ij dO_i      dS_ij = P_ij (dO_i . V_j - D_i)      dK_j = sum_i dS_ij Q_i      dQ_i = sum_j dS_ij K_j
//
// No float atomics (training is bit-reproducible run to run): every output row has ONE owner that sums its contributions in a fixed order.
//   attn_bwd_d_kernel     D_i, one wave per 32 queries.  It runs the MFMA chain that produces dO_i . V_j below with o_i in V's place and
//                         keeps the diagonal, so that where one key carries a whole row (o_i = V_j) the difference dO_i . V_j - D_i is
//                         exactly zero instead of a rounding residue.
//   attn_bwd_dq_kernel    query-stationary, the forward's transposed layout: a wave owns 32 queries (one per lane column) and walks all
//                         keys; S^T = K Q^T and dP^T = V dO^T leave key along a lane's registers, so dS^T is the B operand of
//                         dQ^T += K^T dS^T straight from the accumulator (K^T of the tile from LDS).
//   attn_bwd_dkv_kernel   key-stationary: a wave owns 32 keys (K and V fragments stay in registers as B operands) and walks all queries;
//                         S = Q K^T and dP = dO V^T leave QUERY along a lane's registers, so P and dS are the B operands of
//                         dV^T += dO^T P and dK^T += Q^T dS (dO^T, Q^T, lse and D of the 64-query tile from LDS).
// S is recomputed twice (4 MFMAs of the 36 / 52 per 32 x 32 tile) with the forward's operand order, so its bits -- and with them
// sum_j P_ij = 1 against the stored lse -- are the forward's.  The products over d_v run over channels 16 h + j in lane half h (one
// contiguous 64-byte read per lane); the d_qk = 8 outputs use 8 of the MFMA's 32 rows (the other 24 repeat them and are dropped).
// Ragged edges: loads are clamped to row N - 1; a key >= N gets P = 0 in the dq kernel, a query >= N gets lse = +inf (P = exp(-inf) = 0)
// and D = 0 in the dk/dv kernel, so padding contributes exact zeros; rows >= N are never stored.
// Per launch of the three: HBM bytes ~ B N (8 + 8 + 32 + 32 + 32 + 1 + 1 + 8 + 8 + 32) * 4 once per operand (K / V resp. Q / dO are
// re-read per 128-row workgroup out of L2); FLOP 2 B N^2 (8 + 32 + 8) useful in dq + 2 B N^2 (8 + 32 + 32 + 8) in dk/dv; 2 B N^2 exps.
#include "attn_f32.h"
#include "common.h"

namespace {

constexpr int QT = 64;            // rows of the streamed operand per barrier
constexpr int TP = QT + 1;        // floats per transposed LDS row

struct AttnBwdArgs {
    const float* q; const float* k; const float* v;
    int64_t q_rs, k_rs, v_rs;
    const float* o; const float* dout; const float* lse; float* D;      // o, dO [B,N,32]; lse, D [B,N]
    float* dq; float* dk; float* dv;                                     // [B,N,8], [B,N,8], [B,N,32]
    int N;
};

// row of accumulator register i in lane half h (the 32x32 MFMA's C/D layout; the column is the lane's r)
__device__ __forceinline__ int acc_row(int i, int h) { return (i & 3) + 8 * (i >> 2) + 4 * h; }

__global__ void __launch_bounds__(256, 2) attn_fwd_lse_kernel(AttnF32Args a) {
    __shared__ __attribute__((aligned(16))) char vt[32 * ATTN_VT_PITCH];
    const int64_t row0 = (int64_t)blockIdx.y * a.N;
    a.q += row0 * a.q_rs; a.k += row0 * a.k_rs; a.v += row0 * a.v_rs;
    a.o += row0 * a.o_cs; a.lse += row0;
    attn_f32_body<true>(a, blockIdx.x * 128, vt);
}

// 16 channels 16 h .. 16 h + 15 of a 32-channel row
__device__ __forceinline__ void load16(const float* p, float (&f)[16]) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(p + 4 * g);
        f[4 * g] = t[0]; f[4 * g + 1] = t[1]; f[4 * g + 2] = t[2]; f[4 * g + 3] = t[3];
    }
}

__global__ void __launch_bounds__(256) attn_bwd_d_kernel(AttnBwdArgs a) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int N = a.N;
    const int64_t row0 = (int64_t)blockIdx.y * N;
    const int q = blockIdx.x * 128 + wave * 32 + r;
    const int qc = q < N ? q : N - 1;
    float of[16], dof[16];
    load16(a.o + (row0 + qc) * 32 + 16 * h, of);
    load16(a.dout + (row0 + qc) * 32 + 16 * h, dof);
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(of[j], dof[j], acc, 0, 0, 0);
    // the diagonal: row acc_row(i, h) == r  <=>  h == (r >> 2) & 1 and i == (r & 3) + 4 * (r >> 3)
    float d = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i)
        if (i == (r & 3) + 4 * (r >> 3)) d = acc[i];
    if (q < N && h == ((r >> 2) & 1)) a.D[row0 + q] = d;
}

__global__ void __launch_bounds__(256, 2) attn_bwd_dq_kernel(AttnBwdArgs a) {
    __shared__ float kt[8 * TP];                       // K^T of the key tile
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int N = a.N;
    const int64_t row0 = (int64_t)blockIdx.y * N;
    const float* kbase = a.k + row0 * a.k_rs;
    const float* vbase = a.v + row0 * a.v_rs;
    const int q = blockIdx.x * 128 + wave * 32 + r;
    const int qc = q < N ? q : N - 1;

    float qf[4], dof[16];
    {
        const float* qp = a.q + (row0 + qc) * a.q_rs;
#pragma unroll
        for (int j = 0; j < 4; ++j) qf[j] = qp[2 * j + h];
    }
    load16(a.dout + (row0 + qc) * 32 + 16 * h, dof);
    const float lse = a.lse[row0 + qc], Dq = a.D[row0 + qc];

    f32x16 dqacc;
#pragma unroll
    for (int e = 0; e < 16; ++e) dqacc[e] = 0.f;
    const int skey = tid >> 2, spair = tid & 3;        // K staging: thread -> (key within tile, pair of dims)

    for (int k0 = 0; k0 < N; k0 += QT) {
        __syncthreads();   // previous tile's K^T reads are done
        {
            const int key = k0 + skey;
            const float* kp = kbase + (int64_t)(key < N ? key : N - 1) * a.k_rs + 2 * spair;
            kt[(2 * spair) * TP + skey] = kp[0];
            kt[(2 * spair + 1) * TP + skey] = kp[1];
        }
        __syncthreads();
#pragma unroll
        for (int sub = 0; sub < QT / 32; ++sub) {
            const int kb = k0 + sub * 32;
            if (kb >= N) break;
            const int key = kb + r;
            const int64_t kc = key < N ? key : N - 1;
            // ---- S^T = K . Q^T (the forward's operands in the forward's order)
            f32x16 s;
#pragma unroll
            for (int e = 0; e < 16; ++e) s[e] = 0.f;
            {
                const float* kp = kbase + kc * a.k_rs;
#pragma unroll
                for (int j = 0; j < 4; ++j) s = __builtin_amdgcn_mfma_f32_32x32x2f32(kp[2 * j + h], qf[j], s, 0, 0, 0);
            }
            // ---- dP^T = V . dO^T
            f32x16 dp;
#pragma unroll
            for (int e = 0; e < 16; ++e) dp[e] = 0.f;
            {
                float vf[16];
                load16(vbase + kc * a.v_rs + 16 * h, vf);
#pragma unroll
                for (int j = 0; j < 16; ++j) dp = __builtin_amdgcn_mfma_f32_32x32x2f32(vf[j], dof[j], dp, 0, 0, 0);
            }
            // ---- dS^T = P^T (dP^T - D); keys >= N: exactly zero
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float pij = kb + acc_row(i, h) < N ? __expf(s[i] - lse) : 0.f;
                s[i] = pij * (dp[i] - Dq);
            }
            // ---- dQ^T += K^T . dS^T (rows 8..31 of the product repeat rows 0..7 and are dropped)
#pragma unroll
            for (int i = 0; i < 16; ++i)
                dqacc = __builtin_amdgcn_mfma_f32_32x32x2f32(kt[(r & 7) * TP + sub * 32 + acc_row(i, h)], s[i], dqacc, 0, 0, 0);
        }
    }
    if (q < N) {
        const f32x4 t = {dqacc[0], dqacc[1], dqacc[2], dqacc[3]};       // rows 4 h .. 4 h + 3 of dQ^T, column q
        *reinterpret_cast<f32x4*>(a.dq + (row0 + q) * 8 + 4 * h) = t;
    }
}

__global__ void __launch_bounds__(256, 2) attn_bwd_dkv_kernel(AttnBwdArgs a) {
    __shared__ float dot[32 * TP];                     // dO^T of the query tile
    __shared__ float qt[8 * TP];                       // Q^T
    __shared__ float lse_s[QT], d_s[QT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int N = a.N;
    const int64_t row0 = (int64_t)blockIdx.y * N;
    const int key = blockIdx.x * 128 + wave * 32 + r;
    const int64_t kc = key < N ? key : N - 1;

    float kf[4], vf[16];
    {
        const float* kp = a.k + (row0 + kc) * a.k_rs;
#pragma unroll
        for (int j = 0; j < 4; ++j) kf[j] = kp[2 * j + h];
    }
    load16(a.v + (row0 + kc) * a.v_rs + 16 * h, vf);

    f32x16 dvacc, dkacc;
#pragma unroll
    for (int e = 0; e < 16; ++e) { dvacc[e] = 0.f; dkacc[e] = 0.f; }
    const int srow = tid >> 2, spart = tid & 3;        // staging: thread -> (query within tile, 8 channels of dO / 2 dims of Q)

    for (int q0 = 0; q0 < N; q0 += QT) {
        __syncthreads();   // previous tile's LDS reads are done
        {
            const int qi = q0 + srow;
            const int64_t qc = row0 + (qi < N ? qi : N - 1);
            const float* dp = a.dout + qc * 32 + 8 * spart;
            const f32x4 d0 = *reinterpret_cast<const f32x4*>(dp), d1 = *reinterpret_cast<const f32x4*>(dp + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                dot[(8 * spart + e) * TP + srow] = d0[e];
                dot[(8 * spart + 4 + e) * TP + srow] = d1[e];
            }
            const float* qp = a.q + qc * a.q_rs + 2 * spart;
            qt[(2 * spart) * TP + srow] = qp[0];
            qt[(2 * spart + 1) * TP + srow] = qp[1];
            if (spart == 0) {
                lse_s[srow] = qi < N ? a.lse[qc] : INFINITY;     // a padded query: P = exp(s - inf) = 0
                d_s[srow] = qi < N ? a.D[qc] : 0.f;
            }
        }
        __syncthreads();
#pragma unroll
        for (int sub = 0; sub < QT / 32; ++sub) {
            if (q0 + sub * 32 >= N) break;
            const int col = sub * 32 + r;
            // ---- S = Q . K^T (the forward's products in the forward's order)
            f32x16 s;
#pragma unroll
            for (int e = 0; e < 16; ++e) s[e] = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) s = __builtin_amdgcn_mfma_f32_32x32x2f32(qt[(2 * j + h) * TP + col], kf[j], s, 0, 0, 0);
            // ---- dP = dO . V^T
            f32x16 dp;
#pragma unroll
            for (int e = 0; e < 16; ++e) dp[e] = 0.f;
#pragma unroll
            for (int j = 0; j < 16; ++j) dp = __builtin_amdgcn_mfma_f32_32x32x2f32(dot[(16 * h + j) * TP + col], vf[j], dp, 0, 0, 0);
            // ---- P, dS = P (dP - D); dV^T += dO^T . P, dK^T += Q^T . dS (rows 8..31 of the latter repeat rows 0..7 and are dropped)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int row = sub * 32 + acc_row(i, h);
                const float pij = __expf(s[i] - lse_s[row]);
                const float ds = pij * (dp[i] - d_s[row]);
                dvacc = __builtin_amdgcn_mfma_f32_32x32x2f32(dot[r * TP + row], pij, dvacc, 0, 0, 0);
                dkacc = __builtin_amdgcn_mfma_f32_32x32x2f32(qt[(r & 7) * TP + row], ds, dkacc, 0, 0, 0);
            }
        }
    }
    if (key < N) {
        float* vp = a.dv + (row0 + key) * 32;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 t = {dvacc[4 * g], dvacc[4 * g + 1], dvacc[4 * g + 2], dvacc[4 * g + 3]};
            *reinterpret_cast<f32x4*>(vp + 8 * g + 4 * h) = t;
        }
        const f32x4 t = {dkacc[0], dkacc[1], dkacc[2], dkacc[3]};
        *reinterpret_cast<f32x4*>(a.dk + (row0 + key) * 8 + 4 * h) = t;
    }
}

int check_operands(sr_ctx* ctx, const char* what, const void* q, const void* k, const void* v, int64_t q_rs, int64_t k_rs, int64_t v_rs, int B, int N) {
    if (B <= 0 || N <= 0) return ctx->fail(SR_ERR_INVALID, std::string(what) + ": empty tensor");
    if (B > 65535) return ctx->fail(SR_ERR_INVALID, std::string(what) + ": at most 65535 images per launch");
    if (q_rs < 8 || k_rs < 8 || v_rs < 32) return ctx->fail(SR_ERR_INVALID, std::string(what) + ": row strides must cover 8 (q, k) and 32 (v) channels");
    if (q_rs % 4 || k_rs % 4 || v_rs % 4 || (uintptr_t)q % 16 || (uintptr_t)k % 16 || (uintptr_t)v % 16)
        return ctx->fail(SR_ERR_INVALID, std::string(what) + ": views must be 16-byte aligned");
    return SR_OK;
}

}  // namespace

int attention_fwd_lse_launch(sr_ctx* ctx, const float* q, const float* k, const float* v, int64_t q_rs, int64_t k_rs, int64_t v_rs, int B, int N,
                             float* o, float* lse, hipStream_t st) {
    if (int rc = check_operands(ctx, "attention_fwd_lse", q, k, v, q_rs, k_rs, v_rs, B, N)) return rc;
    if ((uintptr_t)o % 16) return ctx->fail(SR_ERR_INVALID, "attention_fwd_lse: views must be 16-byte aligned");
    const AttnF32Args a{q, k, v, q_rs, k_rs, v_rs, o, 32, lse, N};
    const int rec = ctx->prof_open("attn_fwd_lse<f32>", 2.0 * B * (double)N * N * 40.0, (double)B * N * 81.0 * 4, st);
    hipLaunchKernelGGL(attn_fwd_lse_kernel, dim3((unsigned)((N + 127) / 128), (unsigned)B), dim3(256), 0, st, a);
    ctx->prof_close(rec, st);
    SR_HIP(ctx, hipGetLastError());
    return SR_OK;
}

int attention_bwd_launch(sr_ctx* ctx, const float* q, const float* k, const float* v, const float* o, const float* dout, const float* lse,
                         int64_t q_rs, int64_t k_rs, int64_t v_rs, int B, int N, float* dq, float* dk, float* dv, hipStream_t st) {
    if (int rc = check_operands(ctx, "attention_bwd", q, k, v, q_rs, k_rs, v_rs, B, N)) return rc;
    if ((uintptr_t)o % 16 || (uintptr_t)dout % 16 || (uintptr_t)dq % 16 || (uintptr_t)dk % 16 || (uintptr_t)dv % 16)
        return ctx->fail(SR_ERR_INVALID, "attention_bwd: views must be 16-byte aligned");
    float* D = static_cast<float*>(ctx->arena(ctx->attn_d, sizeof(float) * (size_t)B * N, st));
    if (!D) return SR_ERR_OOM;
    const AttnBwdArgs a{q, k, v, q_rs, k_rs, v_rs, o, dout, lse, D, dq, dk, dv, N};
    const dim3 grid((unsigned)((N + 127) / 128), (unsigned)B);
    const double n2 = (double)B * N * N;
    int rec = ctx->prof_open("attn_bwd_d<f32>", 2.0 * B * (double)N * 32.0, (double)B * N * 65.0 * 4, st);
    hipLaunchKernelGGL(attn_bwd_d_kernel, grid, dim3(256), 0, st, a);
    ctx->prof_close(rec, st);
    rec = ctx->prof_open("attn_bwd_dq<f32>", 2.0 * n2 * 48.0, (double)B * N * (8 + 8 + 32 + 32 + 2 + 8) * 4, st);
    hipLaunchKernelGGL(attn_bwd_dq_kernel, grid, dim3(256), 0, st, a);
    ctx->prof_close(rec, st);
    rec = ctx->prof_open("attn_bwd_dkv<f32>", 2.0 * n2 * 80.0, (double)B * N * (8 + 8 + 32 + 32 + 2 + 8 + 32) * 4, st);
    hipLaunchKernelGGL(attn_bwd_dkv_kernel, grid, dim3(256), 0, st, a);
    ctx->prof_close(rec, st);
    SR_HIP(ctx, hipGetLastError());
    return SR_OK;
}
