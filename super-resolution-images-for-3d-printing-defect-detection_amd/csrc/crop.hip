// crop.hip -- the reference's smart_square_crop (data/common_methods.py:4-49) for B uint8 BGR frames [H, W, 3] of one shape: the square of
// side S = min(W, H) centred on the bounding box of the largest external contour of the Otsu mask.  No contour is traced: with
// RETR_EXTERNAL the contours are the 8-connected components of the hole-filled mask, boundingRect is a component's pixel bounding box and
// contourArea is a sum over 2 x 2 pixel cells (include/sr355.h states the contract, tests/crop_ref.py restates it in NumPy, border follower
// included).  Everything is an integer but Otsu's 256 fp64 steps, which run sequentially and uncontracted; sums are integer atomics, so a
// frame's row is the same bits on every run and for any B.  Nothing comes back to the host between the stages.
//
//   gray, histogram   one workgroup per 4096 pixels: 12-byte loads of four BGR pixels where the frame is 4-byte aligned, one LDS histogram per
//                     wave, merged into the frame's 256 global bins by atomics.
//   Otsu              one thread per frame, OpenCV's getThreshVal_Otsu_8u step for step.  mask = gray > t.
//   labelling         label_tile_kernel / label_seam_kernel / label_compress_kernel<CONN, Pred>: union-find on pixel indices, the parent of
//                     a pixel always a smaller raster index of its own component.  One workgroup per 32 x 32 tile builds the tile's forest in
//                     LDS (each pixel unites with its backward neighbours by atomicMin), flattens it and writes global indices; the seam
//                     kernel unites across tile borders in global memory the same way; the compress kernel replaces every parent by its root.
//                     A pixel's label is then its component's smallest raster index -- the pixel at which Suzuki's raster scan starts that
//                     contour.  Run twice: 4-connected on the background (mask == 0), after which the components holding a pixel of the
//                     frame's border are `outside` (the ring of background OpenCV pads the frame with joins exactly those) and F = not
//                     outside; then 8-connected on F.
//   reductions        twice the area per root: one thread per 2 x 2 cell, lanes of a wave that share a root add up first, one atomic per root
//                     and wave.  The winner per frame is one 64-bit atomicMax of (twice-area, root); its bounding box is a second pass over the
//                     labels (the top row is the root's own).
//   box, gather       the reference's arithmetic per frame, then a row-wise copy at the widest vector both addresses allow.
#include "common.h"

#include <algorithm>
#include <cfloat>
#include <string>

namespace {

constexpr int LT = 32;                          // labelling tile edge: 1024 parents = 4 KB of LDS, four pixels per thread
constexpr int CROP_MAX = 4096;                  // H W <= 2^24: a raster index and twice an area fit an int
constexpr int GH_PIX = 4096;                    // pixels per workgroup of the gray / histogram pass
// max(contours, key=cv2.contourArea) takes the first maximum of a list OpenCV returns last-found first: among equal areas the contour whose
// raster-scan start comes last, i.e. the largest root.  The one point of the contract that is not pinned against OpenCV itself.
constexpr bool TIE_TAKES_LARGEST_ROOT = true;

typedef unsigned long long u64;

inline size_t al256(size_t n) { return (n + 255) & ~(size_t)255; }

struct IsZero { __device__ static bool test(uint8_t v) { return v == 0; } };
struct NonZero { __device__ static bool test(uint8_t v) { return v != 0; } };

// ------------------------------------------------------------------------------------------------
// 1. gray and histogram.  grid (chunks of GH_PIX pixels, B); hist [B][256] zeroed before
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) crop_gray_hist_kernel(const uint8_t* bgr, int HW, uint8_t* gray, int* hist) {
    __shared__ int h[4][256];
    const int b = blockIdx.y, tid = threadIdx.x;
    const uint8_t* img = bgr + (int64_t)b * HW * 3;
    uint8_t* g = gray + (int64_t)b * HW;
    int* hw = h[tid >> 6];
    for (int k = 0; k < 4; ++k) h[k][tid] = 0;
    __syncthreads();
    const int p0 = blockIdx.x * GH_PIX, p1 = min(p0 + GH_PIX, HW);
    if (((((uintptr_t)img) | ((uintptr_t)g)) & 3) == 0) {               // p0 is a multiple of 4: 3 p and p stay 4-byte aligned
        for (int p = p0 + 4 * tid; p < p1; p += 1024) {
            if (p + 4 <= p1) {
                const uint32_t* s = reinterpret_cast<const uint32_t*>(img + 3 * (int64_t)p);      // b0 g0 r0 b1 | g1 r1 b2 g2 | r2 b3 g3 r3
                const uint32_t w0 = s[0], w1 = s[1], w2 = s[2];
                const int g0 = gray_bgr(w0 & 255, (w0 >> 8) & 255, (w0 >> 16) & 255), g1 = gray_bgr(w0 >> 24, w1 & 255, (w1 >> 8) & 255);
                const int g2 = gray_bgr((w1 >> 16) & 255, w1 >> 24, w2 & 255), g3 = gray_bgr((w2 >> 8) & 255, (w2 >> 16) & 255, w2 >> 24);
                *reinterpret_cast<uint32_t*>(g + p) = (uint32_t)g0 | ((uint32_t)g1 << 8) | ((uint32_t)g2 << 16) | ((uint32_t)g3 << 24);
                atomicAdd(&hw[g0], 1);
                atomicAdd(&hw[g1], 1);
                atomicAdd(&hw[g2], 1);
                atomicAdd(&hw[g3], 1);
            } else {
                for (int q = p; q < p1; ++q) {
                    const int gv = gray_bgr(img[3 * (int64_t)q], img[3 * (int64_t)q + 1], img[3 * (int64_t)q + 2]);
                    g[q] = (uint8_t)gv;
                    atomicAdd(&hw[gv], 1);
                }
            }
        }
    } else {
        for (int p = p0 + tid; p < p1; p += 256) {
            const int gv = gray_bgr(img[3 * (int64_t)p], img[3 * (int64_t)p + 1], img[3 * (int64_t)p + 2]);
            g[p] = (uint8_t)gv;
            atomicAdd(&hw[gv], 1);
        }
    }
    __syncthreads();
    const int n = h[0][tid] + h[1][tid] + h[2][tid] + h[3][tid];
    if (n) atomicAdd(&hist[b * 256 + tid], n);
}

// ------------------------------------------------------------------------------------------------
// 2. Otsu: OpenCV 4's getThreshVal_Otsu_8u, one thread per frame, every product and sum rounded on its own -> boxes[b][7]
// ------------------------------------------------------------------------------------------------
__global__ void crop_otsu_kernel(const int* hist, int B, double scale, int* boxes) {
#pragma clang fp contract(off)
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int* h = hist + b * 256;
    double mu = 0.0;
    for (int i = 0; i < 256; ++i) mu += (double)i * (double)h[i];
    mu *= scale;
    double mu1 = 0.0, q1 = 0.0, max_sigma = 0.0;
    int max_val = 0;
    for (int i = 0; i < 256; ++i) {
        const double p = (double)h[i] * scale;
        mu1 *= q1;
        q1 += p;
        const double q2 = 1.0 - q1;
        if (fmin(q1, q2) < (double)FLT_EPSILON || fmax(q1, q2) > 1.0 - (double)FLT_EPSILON) continue;
        mu1 = (mu1 + (double)i * p) / q1;
        const double mu2 = (mu - q1 * mu1) / q2;
        const double d = mu1 - mu2;
        const double sigma = q1 * q2 * d * d;
        if (sigma > max_sigma) { max_sigma = sigma; max_val = i; }
    }
    boxes[b * SR_BOX_COLS + SR_BOX_OTSU] = max_val;
}

// mask = gray > t ? 255 : 0.  grid (chunks, B)
__global__ void __launch_bounds__(256) crop_mask_kernel(const uint8_t* gray, int HW, const int* boxes, uint8_t* mask) {
    const int b = blockIdx.y, t = boxes[b * SR_BOX_COLS + SR_BOX_OTSU];
    const uint8_t* g = gray + (int64_t)b * HW;
    uint8_t* m = mask + (int64_t)b * HW;
    for (int p = blockIdx.x * 256 + threadIdx.x; p < HW; p += gridDim.x * 256) m[p] = g[p] > t ? 255 : 0;
}

// ------------------------------------------------------------------------------------------------
// 3 / 4. labelling.  lab [B][H W]: the parent's raster index, -1 where the predicate fails.  Parents only ever decrease, and a parent is
//        replaced by atomicMin alone, so a reader that sees an older parent still sees a member of the same component that lies above the root.
// ------------------------------------------------------------------------------------------------
__device__ inline int lds_find(volatile int* l, int x) {
    for (int n = l[x]; n != x; n = l[x]) x = n;
    return x;
}

__device__ inline void lds_union(int* l, int a, int b) {
    for (;;) {
        a = lds_find(l, a);
        b = lds_find(l, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }          // a > b: hang a below b
        const int old = atomicMin(&l[a], b);
        if (old == a) return;
        a = old;                                                 // a had a parent already: that parent and b still have to meet
    }
}

__device__ inline int glb_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ inline int glb_find(const int* L, int x) {
    for (int n = glb_load(L + x); n != x; n = glb_load(L + x)) x = n;
    return x;
}

__device__ inline void glb_union(int* L, int a, int b) {
    for (;;) {
        a = glb_find(L, a);
        b = glb_find(L, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&L[a], b);
        if (old == a) return;
        a = old;
    }
}

// grid (tiles x, tiles y, B)
template <int CONN, class Pred>
__global__ void __launch_bounds__(256) label_tile_kernel(const uint8_t* plane, int H, int W, int* lab) {
    __shared__ int l[LT * LT];
    const int tid = threadIdx.x;
    const int y0 = blockIdx.y * LT, x0 = blockIdx.x * LT;
    const int64_t off = (int64_t)blockIdx.z * H * W;
    const uint8_t* P = plane + off;
    int* L = lab + off;
    bool in[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int i = tid + 256 * q, y = y0 + (i >> 5), x = x0 + (i & 31);
        in[q] = y < H && x < W && Pred::test(P[y * W + x]);
        l[i] = in[q] ? i : -1;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (!in[q]) continue;
        const int i = tid + 256 * q, r = i >> 5, c = i & 31;
        if (c > 0 && l[i - 1] >= 0) lds_union(l, i, i - 1);
        if (r > 0) {
            if (l[i - LT] >= 0) lds_union(l, i, i - LT);
            if (CONN == 8) {
                if (c > 0 && l[i - LT - 1] >= 0) lds_union(l, i, i - LT - 1);
                if (c < LT - 1 && l[i - LT + 1] >= 0) lds_union(l, i, i - LT + 1);
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int i = tid + 256 * q, y = y0 + (i >> 5), x = x0 + (i & 31);
        if (y >= H || x >= W) continue;
        int v = -1;
        if (in[q]) {
            const int root = lds_find(l, i);
            v = (y0 + (root >> 5)) * W + x0 + (root & 31);          // the tile's raster order is the frame's: the smallest stays the smallest
        }
        L[y * W + x] = v;
    }
}

// one thread per pixel; only pixels in a tile's first row, first column or last column have a backward neighbour in another tile.  grid (chunks, B)
template <int CONN>
__global__ void __launch_bounds__(256) label_seam_kernel(int H, int W, int* lab) {
    const int HW = H * W;
    int* L = lab + (int64_t)blockIdx.y * HW;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
    const int y = p / W, x = p - y * W;
    const int ty = y & (LT - 1), tx = x & (LT - 1);
    if (ty != 0 && tx != 0 && !(CONN == 8 && tx == LT - 1)) return;
    if (glb_load(L + p) < 0) return;
    if (tx == 0 && x > 0 && glb_load(L + p - 1) >= 0) glb_union(L, p, p - 1);
    if (y > 0) {
        if (ty == 0 && glb_load(L + p - W) >= 0) glb_union(L, p, p - W);
        if (CONN == 8) {
            if ((ty == 0 || tx == 0) && x > 0 && glb_load(L + p - W - 1) >= 0) glb_union(L, p, p - W - 1);
            if ((ty == 0 || tx == LT - 1) && x < W - 1 && glb_load(L + p - W + 1) >= 0) glb_union(L, p, p - W + 1);
        }
    }
}

// grid (chunks, B)
__global__ void __launch_bounds__(256) label_compress_kernel(int HW, int* lab) {
    int* L = lab + (int64_t)blockIdx.y * HW;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
    if (glb_load(L + p) < 0) return;
    const int root = glb_find(L, p);
    __hip_atomic_store(L + p, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // a root never changes here; any other parent only moves up to it
}

// background components that own a pixel of the frame's border: flag[B][H W] (zeroed before), at the root.  grid (chunks of the perimeter, B)
__global__ void __launch_bounds__(256) crop_border_kernel(const int* lab, int H, int W, int* flag) {
    const int64_t off = (int64_t)blockIdx.y * H * W;
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= 2 * W + 2 * H) return;
    int y, x;
    if (k < W) { y = 0; x = k; }
    else if (k < 2 * W) { y = H - 1; x = k - W; }
    else if (k < 2 * W + H) { y = k - 2 * W; x = 0; }
    else { y = k - 2 * W - H; x = W - 1; }
    const int r = lab[off + y * W + x];
    if (r >= 0) flag[off + r] = 1;
}

// F = 255 everywhere but on the outside background.  grid (chunks, B)
__global__ void __launch_bounds__(256) crop_fill_kernel(const int* lab, const int* flag, int HW, uint8_t* filled) {
    const int64_t off = (int64_t)blockIdx.y * HW;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
    const int r = lab[off + p];
    filled[off + p] = (r >= 0 && flag[off + r]) ? 0 : 255;
}

// ------------------------------------------------------------------------------------------------
// 5. reductions keyed by root
// ------------------------------------------------------------------------------------------------
// twice the contour area: the 2 x 2 cell whose top-left pixel is p adds 2 with four pixels of F, 1 with three (they are mutually 8-adjacent: one
// root).  area2 [B][H W] zeroed before.  grid (chunks, B)
__global__ void __launch_bounds__(256) crop_area_kernel(const int* lab, int H, int W, int* area2) {
    const int HW = H * W;
    const int64_t off = (int64_t)blockIdx.y * HW;
    const int* L = lab + off;
    const int p = blockIdx.x * 256 + threadIdx.x;
    int root = -1, add = 0;
    if (p < HW) {
        const int y = p / W, x = p - y * W;
        if (y < H - 1 && x < W - 1) {
            const int a = L[p], b = L[p + 1], c = L[p + W], d = L[p + W + 1];
            const int n = (a >= 0) + (b >= 0) + (c >= 0) + (d >= 0);
            if (n >= 3) { root = max(max(a, b), max(c, d)); add = n - 2; }
        }
    }
    const int lane = threadIdx.x & 63;
    u64 todo = __ballot(root >= 0);
    while (todo) {                                              // wave-uniform: the lanes that share the first waiting lane's root add up
        const int leader = __ffsll((long long)todo) - 1;
        const int lr = __shfl(root, leader);
        const bool mine = root == lr;
        int s = mine ? add : 0;
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if (lane == leader) atomicAdd(&area2[off + lr], s);
        todo &= ~__ballot(mine);
    }
}

// win[b] = max over roots of (twice-area, root) + 1; 0: no pixel of F.  grid (chunks, B)
__global__ void __launch_bounds__(256) crop_winner_kernel(const int* lab, const int* area2, int HW, u64* win) {
    const int64_t off = (int64_t)blockIdx.y * HW;
    const int p = blockIdx.x * 256 + threadIdx.x;
    u64 key = 0;
    if (p < HW && lab[off + p] == p) key = (((u64)(unsigned)area2[off + p] << 32) | (unsigned)(TIE_TAKES_LARGEST_ROOT ? p : ~p)) + 1;
    for (int o = 32; o > 0; o >>= 1) {
        const u64 other = __shfl_xor(key, o);
        key = other > key ? other : key;
    }
    if ((threadIdx.x & 63) == 0 && key) atomicMax(&win[blockIdx.y], key);
}

__device__ inline int winner_root(u64 key) {
    const unsigned lo = (unsigned)(key - 1);
    return (int)(TIE_TAKES_LARGEST_ROOT ? lo : ~lo);
}

// bb[b] = {max (W - 1 - x), max x, max y} over the winner's pixels (zeroed before).  grid (chunks, B)
__global__ void __launch_bounds__(256) crop_bbox_kernel(const int* lab, const u64* win, int H, int W, int* bb) {
    const int HW = H * W;
    const u64 key = win[blockIdx.y];
    if (!key) return;
    const int root = winner_root(key);
    const int p = blockIdx.x * 256 + threadIdx.x;
    int v0 = -1, v1 = -1, v2 = -1;
    if (p < HW && lab[(int64_t)blockIdx.y * HW + p] == root) {
        const int y = p / W, x = p - y * W;
        v0 = W - 1 - x; v1 = x; v2 = y;
    }
    for (int o = 32; o > 0; o >>= 1) {
        v0 = max(v0, __shfl_xor(v0, o));
        v1 = max(v1, __shfl_xor(v1, o));
        v2 = max(v2, __shfl_xor(v2, o));
    }
    if ((threadIdx.x & 63) == 0 && v1 >= 0) {
        int* o = bb + blockIdx.y * 4;
        atomicMax(&o[0], v0);
        atomicMax(&o[1], v1);
        atomicMax(&o[2], v2);
    }
}

// ------------------------------------------------------------------------------------------------
// 6. box: the reference's arithmetic (common_methods.py:19-47) -> boxes[b] = {found, x, y, ww, hh, left, top, otsu_t}
// ------------------------------------------------------------------------------------------------
__global__ void crop_box_kernel(const u64* win, const int* bb, int B, int H, int W, int* boxes) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int S = min(W, H);
    int* o = boxes + b * SR_BOX_COLS;
    const u64 key = win[b];
    int found = 0, x = 0, y = 0, ww = 0, hh = 0, left, top;
    if (key) {
        found = 1;
        y = winner_root(key) / W;                                // the root is the component's first pixel in raster order: its top row
        x = W - 1 - bb[b * 4];
        ww = bb[b * 4 + 1] - x + 1;
        hh = bb[b * 4 + 2] - y + 1;
        const int cx = x + ww / 2, cy = y + hh / 2, half = S / 2;
        left = max(0, cx - half);
        top = max(0, cy - half);
        if (left + S > W) left = W - S;
        if (top + S > H) top = H - S;
        left = max(0, left);
        top = max(0, top);
    } else {
        left = (W - S) / 2;
        top = (H - S) / 2;
    }
    o[0] = found; o[1] = x; o[2] = y; o[3] = ww; o[4] = hh; o[5] = left; o[6] = top;
}

// y[b][r] = x[b][top + r][left .. left + S): one workgroup per row, at the widest of 16 / 4 / 1 bytes that divides the distance between the
// two addresses (the bytes before the first aligned address and after the last whole vector go singly).  left and top are clamped into the
// frame, so that no table can make the copy read outside it.  grid (S, B)
__global__ void __launch_bounds__(256) crop_gather_kernel(const uint8_t* x, int H, int W, int S, const int* boxes, uint8_t* y) {
    const int b = blockIdx.y, r = blockIdx.x, tid = threadIdx.x;
    const int left = min(max(boxes[b * SR_BOX_COLS + SR_BOX_LEFT], 0), W - S), top = min(max(boxes[b * SR_BOX_COLS + SR_BOX_TOP], 0), H - S);
    const uint8_t* s = x + (((int64_t)b * H + top + r) * W + left) * 3;
    uint8_t* d = y + ((int64_t)b * S + r) * S * 3;
    const int n = 3 * S;
    const unsigned diff = (unsigned)((uintptr_t)s - (uintptr_t)d);
    const int v = (diff & 15) == 0 ? 16 : ((diff & 3) == 0 ? 4 : 1);
    const int head = min(n, (int)((v - ((uintptr_t)d & (v - 1))) & (v - 1)));
    const int nv = (n - head) / v, tail0 = head + nv * v;
    for (int i = tid; i < head; i += 256) d[i] = s[i];
    if (v == 16) {
        const uint4* sv = reinterpret_cast<const uint4*>(s + head);
        uint4* dv = reinterpret_cast<uint4*>(d + head);
        for (int i = tid; i < nv; i += 256) dv[i] = sv[i];
    } else if (v == 4) {
        const uint32_t* sv = reinterpret_cast<const uint32_t*>(s + head);
        uint32_t* dv = reinterpret_cast<uint32_t*>(d + head);
        for (int i = tid; i < nv; i += 256) dv[i] = sv[i];
    } else {
        for (int i = head + tid; i < tail0; i += 256) d[i] = s[i];
    }
    for (int i = tail0 + tid; i < n; i += 256) d[i] = s[i];
}

int check_frames(sr_ctx* ctx, const char* who, int B, int H, int W) {
    if (B < 1 || B > 32767) return ctx->fail(SR_ERR_INVALID, std::string(who) + ": empty or oversized batch (1 <= B <= 32767)");
    if (H < 2 || W < 2 || H > CROP_MAX || W > CROP_MAX)
        return ctx->fail(SR_ERR_INVALID, std::string(who) + ": H and W must lie in 2 .. 4096, got " + std::to_string(H) + " x " + std::to_string(W));
    return SR_OK;
}

template <int CONN, class Pred>
void label_components(const uint8_t* plane, int B, int H, int W, int* lab, hipStream_t st) {
    const int HW = H * W;
    const dim3 pgrid((HW + 255) / 256, B);
    hipLaunchKernelGGL((label_tile_kernel<CONN, Pred>), dim3((W + LT - 1) / LT, (H + LT - 1) / LT, B), dim3(256), 0, st, plane, H, W, lab);
    hipLaunchKernelGGL(label_seam_kernel<CONN>, pgrid, dim3(256), 0, st, H, W, lab);
    hipLaunchKernelGGL(label_compress_kernel, pgrid, dim3(256), 0, st, HW, lab);
}

}  // namespace

extern "C" {

int sr_object_boxes(sr_ctx* ctx, const uint8_t* bgr_u8, int B, int H, int W, int32_t* boxes_i32, uint8_t* gray_u8, uint8_t* mask_u8, int32_t* labels_i32,
                    void* stream) {
    DeviceGuard dg_(ctx);
    if (!ctx) return SR_ERR_INVALID;
    if (!bgr_u8 || !boxes_i32) return ctx->fail(SR_ERR_INVALID, "object_boxes: null tensor");
    if (int rc = check_frames(ctx, "object_boxes", B, H, W)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int HW = H * W;
    const size_t n = (size_t)B * HW;
    const size_t b_small = al256(sizeof(int) * (size_t)B * 256) + al256(sizeof(u64) * (size_t)B) + al256(sizeof(int) * (size_t)B * 4);
    const size_t b_u8 = al256(n), b_i32 = al256(sizeof(int) * n);
    char* wk = static_cast<char*>(ctx->arena(ctx->crop_work, b_small + (gray_u8 ? 0 : b_u8) + (mask_u8 ? 0 : b_u8) + b_u8 + (labels_i32 ? 0 : b_i32) + b_i32, st));
    if (!wk) return SR_ERR_OOM;
    char* small = wk;
    int* hist = reinterpret_cast<int*>(wk); wk += al256(sizeof(int) * (size_t)B * 256);
    u64* win = reinterpret_cast<u64*>(wk); wk += al256(sizeof(u64) * (size_t)B);
    int* bb = reinterpret_cast<int*>(wk); wk += al256(sizeof(int) * (size_t)B * 4);
    uint8_t* gray = gray_u8 ? gray_u8 : reinterpret_cast<uint8_t*>(wk); wk += gray_u8 ? 0 : b_u8;
    uint8_t* mask = mask_u8 ? mask_u8 : reinterpret_cast<uint8_t*>(wk); wk += mask_u8 ? 0 : b_u8;
    uint8_t* filled = reinterpret_cast<uint8_t*>(wk); wk += b_u8;
    int* lab = labels_i32 ? labels_i32 : reinterpret_cast<int*>(wk); wk += labels_i32 ? 0 : b_i32;
    int* aux = reinterpret_cast<int*>(wk);                      // the border flags of the background pass, then twice the areas

    const dim3 pgrid((HW + 255) / 256, B);
    const dim3 sgrid((unsigned)std::min((HW + 255) / 256, 1024), B);
    SR_HIP(ctx, hipMemsetAsync(small, 0, b_small, st));
    int rec = ctx->prof_open("crop_gray_otsu", 0.0, (double)n * 5.0, st);
    hipLaunchKernelGGL(crop_gray_hist_kernel, dim3((HW + GH_PIX - 1) / GH_PIX, B), dim3(256), 0, st, bgr_u8, HW, gray, hist);
    hipLaunchKernelGGL(crop_otsu_kernel, dim3((B + 63) / 64), dim3(64), 0, st, hist, B, 1.0 / (double)HW, boxes_i32);
    hipLaunchKernelGGL(crop_mask_kernel, sgrid, dim3(256), 0, st, gray, HW, boxes_i32, mask);
    ctx->prof_close(rec, st);

    rec = ctx->prof_open("crop_label_background", 0.0, 0.0, st);
    SR_HIP(ctx, hipMemsetAsync(aux, 0, sizeof(int) * n, st));
    label_components<4, IsZero>(mask, B, H, W, lab, st);
    hipLaunchKernelGGL(crop_border_kernel, dim3((2 * W + 2 * H + 255) / 256, B), dim3(256), 0, st, lab, H, W, aux);
    hipLaunchKernelGGL(crop_fill_kernel, pgrid, dim3(256), 0, st, lab, aux, HW, filled);
    ctx->prof_close(rec, st);

    rec = ctx->prof_open("crop_label_filled", 0.0, 0.0, st);
    label_components<8, NonZero>(filled, B, H, W, lab, st);
    ctx->prof_close(rec, st);

    rec = ctx->prof_open("crop_reduce", 0.0, 0.0, st);
    SR_HIP(ctx, hipMemsetAsync(aux, 0, sizeof(int) * n, st));
    hipLaunchKernelGGL(crop_area_kernel, pgrid, dim3(256), 0, st, lab, H, W, aux);
    hipLaunchKernelGGL(crop_winner_kernel, pgrid, dim3(256), 0, st, lab, aux, HW, win);
    hipLaunchKernelGGL(crop_bbox_kernel, pgrid, dim3(256), 0, st, lab, win, H, W, bb);
    hipLaunchKernelGGL(crop_box_kernel, dim3((B + 63) / 64), dim3(64), 0, st, win, bb, B, H, W, boxes_i32);
    ctx->prof_close(rec, st);
    SR_HIP(ctx, hipGetLastError());
    return SR_OK;
}

int sr_square_crop(sr_ctx* ctx, const uint8_t* bgr_u8, int B, int H, int W, const int32_t* boxes_i32, uint8_t* y_u8, void* stream) {
    DeviceGuard dg_(ctx);
    if (!ctx) return SR_ERR_INVALID;
    if (!bgr_u8 || !boxes_i32 || !y_u8) return ctx->fail(SR_ERR_INVALID, "square_crop: null tensor");
    if (int rc = check_frames(ctx, "square_crop", B, H, W)) return rc;
    if (bgr_u8 == y_u8) return ctx->fail(SR_ERR_INVALID, "square_crop: the crop cannot run in place");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int S = std::min(W, H);
    const int rec = ctx->prof_open("crop_gather", 0.0, 6.0 * B * (double)S * S, st);
    hipLaunchKernelGGL(crop_gather_kernel, dim3(S, B), dim3(256), 0, st, bgr_u8, H, W, S, boxes_i32, y_u8);
    ctx->prof_close(rec, st);
    SR_HIP(ctx, hipGetLastError());
    return SR_OK;
}

}  // extern "C"
