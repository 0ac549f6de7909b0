// disc_train.hip -- the discriminator's own work inside ESRGAN._train_step (reference ESRGAN_model.py:347-377, :475-533) that is not a conv:
// tfa's SpectralNormalization of the eight wrapped kernels where they lie in the trainer's flat parameter bucket, and the dense head
// GAP -> Dense 256 LeakyReLU(0.2) -> Dense 1 sigmoid with Keras' binary cross-entropy, forward and backward.  The host restatements are
// sr355/gan_train.py spectral_normalize / discriminator_forward / bce_mean; both kernels sum in fp64 as the host does.
//
//   sr_spectral_norm_bucket: ONE launch, one workgroup of 16 waves per layer.  With w = kernel.reshape(K, Cout):
//     1. rows: a wave per row k, lanes over Cout (coalesced): t[k] = sum_c u[c] w[k,c]; then |t|^2.
//     2. columns: a wave owns a 64-column tile and every KG-th row (KG = 16 / tiles), lanes over the columns (coalesced):
//        part[kg][c] = sum_k t[k] w[k,c]; the KG partial sums of a column are added in kg order.  v = t / |t| is never formed: v w = (t w) / |t|.
//     3. u' = l2n(v w), sigma = (v w) . u' -- tfa's v w u'^T without a third pass over w -- then kernel[i] = kernel[i] / float(sigma) and u = u'.
//     t and part live in a per-layer slice of a context arena (K + 16 Cout doubles, L2-resident); LDS holds only the 16 wave sums of a
//     workgroup-wide reduction.  Every sum has a fixed order (xor butterfly inside a wave, wave order across waves): no atomics, the same bits
//     on every run.
//   sr_disc_head_step: two launches, after sr_dense_head_step.
//     1. rows: one workgroup of 256 threads per batch row.  g = mean_{H,W} h (thread j = channel j, positions in order), z1 = g k1 + b1
//        (thread j = unit j, k1 read coalesced), a1 = lrelu(z1), z2 = a1 k2 + b2, p = sigmoid(z2), the row's clipped BCE and dz2, dz1,
//        dg = dz1 k1^T (a wave per input channel, lanes over the units) and dh = dg / (H W) written to every position of the row's map.
//     2. grads: one thread per parameter of the head's slice of the flat gradient bucket (kernel, bias, kernel, bias -- train.ParamBucket's
//        order), the batch rows summed in row order, stored or added onto what is there; thread 0 also writes the mean loss.
#include "common.h"
#include "fp_sep.h"

#include <algorithm>
#include <cmath>
#include <utility>

namespace {

constexpr int SN_THREADS = 1024, SN_WAVES = SN_THREADS / 64;
constexpr int DH = 256;               // the head's widths: GAP 256 -> Dense 256 -> Dense 1

struct SnJob {
    int64_t koff, uoff, woff;         // kernel in the bucket, u in the u tensor (floats); t / part in the work arena (doubles)
    int K, Cout;
};

__device__ __forceinline__ double wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// sum of v over the workgroup, the same bits in every thread: butterfly per wave, then the wave sums in wave order
__device__ __forceinline__ double block_sum(double v, double* sred, int nwaves) {
    v = wave_sum(v);
    __syncthreads();                  // the previous reduction's readers are done with sred
    if ((threadIdx.x & 63) == 0) sred[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    for (int i = 0; i < nwaves; ++i) s += sred[i];
    return s;
}

__global__ void __launch_bounds__(SN_THREADS) spectral_norm_kernel(float* __restrict__ bucket, float* __restrict__ uall, const SnJob* __restrict__ jobs,
                                                                   double* __restrict__ work) {
    __shared__ double sred[SN_WAVES];
    const SnJob job = jobs[blockIdx.x];
    const int K = job.K, Cout = job.Cout;
    float* w = bucket + job.koff;
    float* u = uall + job.uoff;
    double* t = work + job.woff;                  // [K]
    double* part = t + K;                         // [SN_WAVES][Cout]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    // 1. t = u w^T
    for (int k = wave; k < K; k += SN_WAVES) {
        const float* row = w + (int64_t)k * Cout;
        double a = 0.0;
        for (int c = lane; c < Cout; c += 64) a = fma((double)u[c], (double)row[c], a);
        a = wave_sum(a);
        if (lane == 0) t[k] = a;
    }
    __syncthreads();
    double q = 0.0;
    for (int k = tid; k < K; k += SN_THREADS) q = fma(t[k], t[k], q);
    const double nt = sqrt(fmax(block_sum(q, sred, SN_WAVES), 1e-12));

    // 2. part[kg] = the rows kg, kg + KG, ... of t w
    const int tiles = (Cout + 63) / 64;
    const int KG = tiles >= SN_WAVES ? 1 : SN_WAVES / tiles;
    const int kg = tiles >= SN_WAVES ? 0 : wave / tiles;
    if (kg < KG) {
        for (int tile = tiles >= SN_WAVES ? wave : wave % tiles; tile < tiles; tile += SN_WAVES) {
            const int c = tile * 64 + lane;
            if (c < Cout) {
                double a = 0.0;
                for (int k = kg; k < K; k += KG) a = fma(t[k], (double)w[(int64_t)k * Cout + c], a);
                part[(int64_t)kg * Cout + c] = a;
            }
        }
    }
    __syncthreads();

    // 3. v w, u' = l2n(v w), sigma = (v w) . u'
    double q2 = 0.0;
    for (int c = tid; c < Cout; c += SN_THREADS) {
        double s = 0.0;
        for (int g = 0; g < KG; ++g) s += part[(int64_t)g * Cout + c];
        s /= nt;
        part[c] = s;                              // this thread's column only
        q2 = fma(s, s, q2);
    }
    const double nu = sqrt(fmax(block_sum(q2, sred, SN_WAVES), 1e-12));
    double sg = 0.0;
    for (int c = tid; c < Cout; c += SN_THREADS) {
        const double vw = part[c], un = vw / nu;
        sg = fma(vw, un, sg);
        u[c] = (float)un;
    }
    const float sigma = (float)block_sum(sg, sred, SN_WAVES);
    const int64_t n = (int64_t)K * Cout;
    for (int64_t i = tid; i < n; i += SN_THREADS) w[i] = __fdiv_rn(w[i], sigma);
}

struct DiscHeadWork {
    double *g, *a1, *dz1, *dz2, *loss;            // [B,256] [B,256] [B,256] [B] [B]
};

size_t dh_align(size_t b) { return (b + 255) / 256 * 256; }

size_t disc_head_work_bytes(int B) { return 3 * dh_align(sizeof(double) * (size_t)B * DH) + 2 * dh_align(sizeof(double) * (size_t)B); }

DiscHeadWork disc_head_work(void* p0, int B) {
    char* p = static_cast<char*>(p0);
    DiscHeadWork k;
    k.g = reinterpret_cast<double*>(p); p += dh_align(sizeof(double) * (size_t)B * DH);
    k.a1 = reinterpret_cast<double*>(p); p += dh_align(sizeof(double) * (size_t)B * DH);
    k.dz1 = reinterpret_cast<double*>(p); p += dh_align(sizeof(double) * (size_t)B * DH);
    k.dz2 = reinterpret_cast<double*>(p); p += dh_align(sizeof(double) * (size_t)B);
    k.loss = reinterpret_cast<double*>(p);
    return k;
}

__global__ void __launch_bounds__(DH) disc_head_rows_kernel(const float* __restrict__ h, int B, int HW, const float* __restrict__ prm, float target,
                                                            float* __restrict__ p_out, float* __restrict__ dh, DiscHeadWork wk) {
    const float* k1 = prm;
    const float* b1 = k1 + DH * DH;
    const float* k2 = b1 + DH;
    const float* b2 = k2 + DH;
    __shared__ double sv[DH];                     // g, then dz1
    __shared__ double sdg[DH];
    __shared__ double sred[DH / 64];
    const int b = blockIdx.x, j = threadIdx.x, lane = j & 63, wave = j >> 6;
    const float* hb = h + (int64_t)b * HW * DH;

    double g = 0.0;
    for (int p = 0; p < HW; ++p) g += (double)hb[(int64_t)p * DH + j];
    g /= (double)HW;
    sv[j] = g;
    wk.g[(int64_t)b * DH + j] = g;
    __syncthreads();

    double z1 = 0.0;
    for (int i = 0; i < DH; ++i) z1 = fma(sv[i], (double)k1[i * DH + j], z1);
    z1 += (double)b1[j];
    const double a1 = z1 > 0.0 ? z1 : 0.2 * z1;
    wk.a1[(int64_t)b * DH + j] = a1;
    const double z2 = block_sum(a1 * (double)k2[j], sred, DH / 64) + (double)b2[0];
    const double p = 1.0 / (1.0 + exp(-z2));

    // keras.backend.binary_crossentropy on probabilities: clip to [eps, 1 - eps], + eps inside both logs; the clip passes the gradient inside its range
    const double eps = 1e-7, tg = (double)target;
    const double pc = fmin(fmax(p, eps), 1.0 - eps);
    const double inside = (p >= eps && p <= 1.0 - eps) ? 1.0 : 0.0;
    const double dp = -(tg / (pc + eps) - (1.0 - tg) / (1.0 - pc + eps)) * inside / (double)B;
    const double dz2 = dp * p * (1.0 - p);
    if (j == 0) {
        wk.loss[b] = -(tg * log(pc + eps) + (1.0 - tg) * log(1.0 - pc + eps));
        wk.dz2[b] = dz2;
        p_out[b] = (float)p;
    }
    const double da1 = dz2 * (double)k2[j];
    const double dz1 = z1 > 0.0 ? da1 : 0.2 * da1;
    wk.dz1[(int64_t)b * DH + j] = dz1;
    __syncthreads();                              // every z1 has read g
    sv[j] = dz1;
    __syncthreads();

    // dg[i] = sum_j dz1[j] k1[i,j]: a wave per input channel, lanes over the units
    for (int i = wave; i < DH; i += DH / 64) {
        double a = 0.0;
        for (int q = lane; q < DH; q += 64) a = fma(sv[q], (double)k1[i * DH + q], a);
        a = wave_sum(a);
        if (lane == 0) sdg[i] = a;
    }
    __syncthreads();
    const float d = (float)(sdg[j] / (double)HW);
    float* db = dh + (int64_t)b * HW * DH;
    for (int p_ = 0; p_ < HW; ++p_) db[(int64_t)p_ * DH + j] = d;
}

// one thread per parameter of the head's slice of the gradient bucket; grads == nullptr: the loss only
__global__ void __launch_bounds__(256) disc_head_grads_kernel(int B, DiscHeadWork wk, float* __restrict__ grads, int accumulate, float* __restrict__ loss_out) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e == 0) {
        double l = 0.0;
        for (int r = 0; r < B; ++r) l += wk.loss[r];
        *loss_out = (float)(l / (double)B);
    }
    if (!grads) return;
    constexpr int nk1 = DH * DH, nb1 = DH, nk2 = DH;
    double s = 0.0;
    if (e < nk1) {
        const int i = e / DH, j = e - i * DH;
        for (int r = 0; r < B; ++r) s = fma(wk.g[(int64_t)r * DH + i], wk.dz1[(int64_t)r * DH + j], s);
    } else if (e < nk1 + nb1) {
        const int j = e - nk1;
        for (int r = 0; r < B; ++r) s += wk.dz1[(int64_t)r * DH + j];
    } else if (e < nk1 + nb1 + nk2) {
        const int j = e - nk1 - nb1;
        for (int r = 0; r < B; ++r) s = fma(wk.a1[(int64_t)r * DH + j], wk.dz2[r], s);
    } else if (e == nk1 + nb1 + nk2) {
        for (int r = 0; r < B; ++r) s += wk.dz2[r];
    } else {
        return;
    }
    grads[e] = accumulate ? add_sep(grads[e], (float)s) : (float)s;
}

}  // namespace

extern "C" {

int sr_spectral_norm_bucket(sr_ctx* ctx, float* bucket, int64_t bucket_len, float* u, int64_t u_len, const sr_sn_desc* descs, int n_layers, void* stream) {
    DeviceGuard dg_(ctx);
    if (!ctx) return SR_ERR_INVALID;
    if (!bucket || !u || !descs) return ctx->fail(SR_ERR_INVALID, "spectral_norm_bucket: null pointer");
    if (n_layers <= 0 || n_layers > 65535) return ctx->fail(SR_ERR_INVALID, "spectral_norm_bucket: need 1 <= n_layers <= 65535");
    std::vector<SnJob> jobs((size_t)n_layers);
    int64_t woff = 0;
    for (int i = 0; i < n_layers; ++i) {
        const sr_sn_desc& d = descs[i];
        if (d.K < 1 || d.Cout < 1 || d.koff < 0 || d.uoff < 0) return ctx->fail(SR_ERR_INVALID, "spectral_norm_bucket: a descriptor needs K >= 1, Cout >= 1 and offsets >= 0");
        const int64_t n = (int64_t)d.K * d.Cout;
        if (d.koff > bucket_len || n > bucket_len - d.koff) return ctx->fail(SR_ERR_INVALID, "spectral_norm_bucket: a descriptor reaches past the bucket");
        if (d.uoff > u_len || d.Cout > u_len - d.uoff) return ctx->fail(SR_ERR_INVALID, "spectral_norm_bucket: a descriptor reaches past the u tensor");
        jobs[(size_t)i] = SnJob{d.koff, d.uoff, woff, d.K, d.Cout};
        woff += (int64_t)d.K + (int64_t)SN_WAVES * d.Cout;
    }
    // every layer is its own workgroup: two that shared a float of the bucket or of u would race
    for (int which = 0; which < 2; ++which) {
        std::vector<std::pair<int64_t, int64_t>> spans((size_t)n_layers);
        for (int i = 0; i < n_layers; ++i)
            spans[(size_t)i] = which ? std::make_pair(descs[i].uoff, (int64_t)descs[i].Cout) : std::make_pair(descs[i].koff, (int64_t)descs[i].K * descs[i].Cout);
        std::sort(spans.begin(), spans.end());
        for (size_t i = 1; i < spans.size(); ++i)
            if (spans[i - 1].first + spans[i - 1].second > spans[i].first)
                return ctx->fail(SR_ERR_INVALID, which ? "spectral_norm_bucket: two descriptors' u ranges overlap" : "spectral_norm_bucket: two descriptors' kernels overlap");
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    double* work = static_cast<double*>(ctx->arena(ctx->sn_work, sizeof(double) * (size_t)woff, st));
    const size_t tbytes = sizeof(SnJob) * jobs.size();
    void* tab = ctx->arena(ctx->sn_tab, tbytes, st);
    if (!work || !tab) return SR_ERR_OOM;
    if (ctx->sn_tab_host.size() != tbytes || ctx->sn_tab_dev != tab || memcmp(ctx->sn_tab_host.data(), jobs.data(), tbytes) != 0) {
        SR_HIP(ctx, hipStreamSynchronize(st));                         // an earlier launch may still be reading the old table
        SR_HIP(ctx, hipMemcpy(tab, jobs.data(), tbytes, hipMemcpyHostToDevice));
        ctx->sn_tab_host.assign(reinterpret_cast<const char*>(jobs.data()), reinterpret_cast<const char*>(jobs.data()) + tbytes);
        ctx->sn_tab_dev = tab;
    }
    hipLaunchKernelGGL(spectral_norm_kernel, dim3((unsigned)n_layers), dim3(SN_THREADS), 0, st, bucket, u, static_cast<const SnJob*>(tab), work);
    SR_HIP(ctx, hipGetLastError());
    return SR_OK;
}

int sr_disc_head_step(sr_ctx* ctx, const float* h, int B, int H, int W, int in_dim, int hidden, int out_dim, const float* params, float target,
                      float* loss, float* p, float* dh, float* grads, int accumulate, void* stream) {
    DeviceGuard dg_(ctx);
    if (!ctx) return SR_ERR_INVALID;
    if (!h || !params || !loss || !p || !dh) return ctx->fail(SR_ERR_INVALID, "disc_head_step: null tensor");
    if (in_dim != DH || hidden != DH || out_dim != 1) return ctx->fail(SR_ERR_INVALID, "disc_head_step: the head is GAP 256 -> Dense 256 -> Dense 1");
    if (B < 1 || B > 65535 || H < 1 || W < 1 || (int64_t)B * H * W * DH >= ((int64_t)1 << 31))
        return ctx->fail(SR_ERR_INVALID, "disc_head_step: need 1 <= B <= 65535 and a map of fewer than 2^31 values");
    if (target != 0.f && target != 1.f) return ctx->fail(SR_ERR_INVALID, "disc_head_step: the target is 0 or 1");
    hipStream_t st = static_cast<hipStream_t>(stream);
    void* work = ctx->arena(ctx->dhead_work, disc_head_work_bytes(B), st);
    if (!work) return SR_ERR_OOM;
    const DiscHeadWork wk = disc_head_work(work, B);
    hipLaunchKernelGGL(disc_head_rows_kernel, dim3((unsigned)B), dim3(DH), 0, st, h, B, H * W, params, target, p, dh, wk);
    SR_HIP(ctx, hipGetLastError());
    const unsigned gg = grads ? (unsigned)((DH * DH + DH + DH + 1 + 255) / 256) : 1u;
    hipLaunchKernelGGL(disc_head_grads_kernel, dim3(gg), dim3(256), 0, st, B, wk, grads, accumulate, loss);
    SR_HIP(ctx, hipGetLastError());
    return SR_OK;
}

}  // extern "C"
