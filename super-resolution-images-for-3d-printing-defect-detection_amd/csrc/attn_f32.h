// attn_f32.h -- the fp32 streaming-softmax forward of SelfAttention (ESRGAN_model.py:57-65), stated once for its two kernels:
// attn_f32_kernel (attention.hip, inference: q | k | v are channel ranges of one buffer) and attn_fwd_lse_kernel
// (attention_train.hip, training: three operands of their own, and the per-query softmax statistic the backward pass needs).
// See attention.hip's header for the transposed formulation and the lane layout.
#pragma once
#include "common.h"

constexpr int ATTN_KV_TILE = 64;                          // keys per barrier
constexpr int ATTN_VT_PITCH = ATTN_KV_TILE * 4 + 4;       // bytes per V^T row in LDS

// Operands as pointer + row stride in elements, already advanced to the image; o is [N][o_cs] with the 32 channels at the pointer.
struct AttnF32Args {
    const float* q; const float* k; const float* v;
    int64_t q_rs, k_rs, v_rs;
    float* o; int64_t o_cs;
    float* lse;               // LSE only: [N], m + log(l) in natural log
    int N;
};

__device__ __forceinline__ float attn_xhalf(float v) { return __shfl_xor(v, 32); }

// One workgroup = 4 waves = 128 queries starting at q0; exact fp32 MFMA (32x32x2_f32) for both products, one 32-query block per wave.
// vt: 32 * ATTN_VT_PITCH bytes of LDS.  LSE = false is the inference kernel, whose arithmetic LSE = true repeats operation for operation.
template <bool LSE>
__device__ __forceinline__ void attn_f32_body(const AttnF32Args& a, const int q0, char* vt) {
    constexpr int PITCH = ATTN_VT_PITCH;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int N = a.N;
    const int q = q0 + wave * 32 + r;
    const int qc = q < N ? q : N - 1;

    // query fragment (B operand of S^T = K.Q^T)
    float qf[4];
    {
        const float* qp = a.q + (int64_t)qc * a.q_rs;
#pragma unroll
        for (int j = 0; j < 4; ++j) qf[j] = qp[2 * j + h];
    }

    f32x16 oacc;
#pragma unroll
    for (int e = 0; e < 16; ++e) oacc[e] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;

    // V staging assignment: thread -> (key within tile, 8-channel octet)
    const int skey = tid >> 2, soct = tid & 3;

    for (int k0 = 0; k0 < N; k0 += ATTN_KV_TILE) {
        __syncthreads();   // previous tile's V^T reads are done
        {
            const int key = k0 + skey;
            const float* vp = a.v + (int64_t)(key < N ? key : N - 1) * a.v_rs + soct * 8;
            f32x4 v0 = *reinterpret_cast<const f32x4*>(vp), v1 = *reinterpret_cast<const f32x4*>(vp + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                *reinterpret_cast<float*>(vt + (soct * 8 + e) * PITCH + skey * 4) = v0[e];
                *reinterpret_cast<float*>(vt + (soct * 8 + 4 + e) * PITCH + skey * 4) = v1[e];
            }
        }
        __syncthreads();
#pragma unroll
        for (int sub = 0; sub < ATTN_KV_TILE / 32; ++sub) {
            const int kb = k0 + sub * 32;
            if (kb >= N) break;
            // ---- S^T = K . Q^T
            f32x16 s;
#pragma unroll
            for (int e = 0; e < 16; ++e) s[e] = 0.f;
            {
                const int key = kb + r;
                const float* kp = a.k + (int64_t)(key < N ? key : N - 1) * a.k_rs;
#pragma unroll
                for (int j = 0; j < 4; ++j) s = __builtin_amdgcn_mfma_f32_32x32x2f32(kp[2 * j + h], qf[j], s, 0, 0, 0);
            }
            // ---- online softmax over this tile's 32 keys (16 here, 16 in lane^32)
            float mx = -INFINITY;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int key = kb + (i & 3) + 8 * (i >> 2) + 4 * h;
                if (key >= N) s[i] = -INFINITY;
                mx = fmaxf(mx, s[i]);
            }
            mx = fmaxf(mx, attn_xhalf(mx));
            const float m_new = fmaxf(m_run, mx);          // finite: every tile has >= 1 live key
            const float alpha = __expf(m_run - m_new);     // exp(-inf) = 0 on the first tile
            float psum = 0.f;
#pragma unroll
            for (int i = 0; i < 16; ++i) { s[i] = __expf(s[i] - m_new); psum += s[i]; }
            l_run = l_run * alpha + psum;
            m_run = m_new;
#pragma unroll
            for (int e = 0; e < 16; ++e) oacc[e] *= alpha;
            // ---- O^T += V^T . P^T
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int krow = sub * 32 + (i & 3) + 8 * (i >> 2);
                const float va = *reinterpret_cast<const float*>(vt + r * PITCH + (krow + 4 * h) * 4);
                oacc = __builtin_amdgcn_mfma_f32_32x32x2f32(va, s[i], oacc, 0, 0, 0);
            }
        }
    }
    const float l_tot = l_run + attn_xhalf(l_run);
    const float inv = 1.f / l_tot;
    if (q < N) {
        float* op = a.o + (int64_t)q * a.o_cs;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int d0 = 8 * g + 4 * h;
            f32x4 t = {oacc[4 * g] * inv, oacc[4 * g + 1] * inv, oacc[4 * g + 2] * inv, oacc[4 * g + 3] * inv};
            *reinterpret_cast<f32x4*>(op + d0) = t;
        }
        if constexpr (LSE) {
            if (h == 0) a.lse[q] = m_run + logf(l_tot);
        }
    }
}
