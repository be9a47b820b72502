// ranenv_ppo_parts.hpp -- the device functions the training kernels share (ranenv_ppo.hip: the PPO updates; ranenv_sac.hip: the SAC
// update): the LDS size of a net's rows, the backward pass of one 32-row tile on the f32 matrix cores, the workgroup sum in slot order,
// Adam's float32 step and the bias corrections' powers.  ranenv_ppo.hip's header comment describes the plan they belong to; the text
// is what stood there, so the kernels built from it keep their instructions.
#pragma once
#include "ranenv_net.hpp"

namespace {

// Floats of LDS for the rows of `net`: the input and every layer's output, 32 rows each
__host__ __device__ inline int ppo_act_floats(const PolicyNet &net)
{
    int n = NET_ROWS * net_ld(net.kp[0]);
    for (int l = 0; l < net.n_layers; l++) n += NET_ROWS * net_ld(net.np[l]);
    return n;
}

// ---- the wide plan (ranenv_ppo_bind_wide): two row buffers in LDS, every layer's input rows parked in the workgroup's scratch --------
// Rows array j of a net -- 0 its input, j >= 1 layer j - 1's output -- lies in the buffer that grows up from `base` (even j) or in the
// one that ends at `top` (odd j), `top` - `base` = ppo_wide_floats(net): arrays j and j + 1, the only two alive at a time, never meet.
__host__ __device__ inline int ppo_wide_floats(const PolicyNet &net)
{
    int n = 0;
    for (int l = 0; l < net.n_layers; l++) { const int v = NET_ROWS * (net_ld(net.kp[l]) + net_ld(net.np[l])); n = v > n ? v : n; }
    return n;
}
// Floats of scratch for the parked rows of `net`: slab l = layer l's 32 input rows at stride net_ld(kp[l]), back to back
__host__ __device__ inline long long ppo_wide_scratch_floats(const PolicyNet &net)
{
    long long n = 0;
    for (int l = 0; l < net.n_layers; l++) n += NET_ROWS * net_ld(net.kp[l]);
    return n;
}
__device__ __forceinline__ float *ppo_wide_buf(const PolicyNet &net, int j, float *base, float *top)
{
    return (j & 1) ? top - NET_ROWS * net_ld(j == 0 ? net.kp[0] : net.np[j - 1]) : base;
}
// 32 rows x K columns at stride net_ld(K) from `src` to `dst` (LDS to scratch or back): a float4 per thread at a lane-dependent address
__device__ __forceinline__ void ppo_copy_rows(float *dst, const float *src, int K, int tid)
{
    const int ld = net_ld(K), kq = K >> 2;
    for (int i = tid; i < NET_ROWS * kq; i += 256) {
        const int r = i / kq, at = r * ld + ((i - r * kq) << 2);
        *(float4 *)(dst + at) = *(const float4 *)(src + at);
    }
}

// The backward pass of one tile: `out` = the output layer's rows, holding dL/d(output); the layers' inputs lie in front of it (see
// ranenv_ppo.hip's header).  Adds the tile's share to the packed gradient `g`; reads the weights `w`.  Ends without a barrier.
// WIDE: layer l's input rows A come back from slab l of `park` into the buffer dZ does not hold (a barrier behind the load; the
// buffer is free: what it held, the dZ of layer l + 1, was last read in front of that layer's closing barrier), the arithmetic is the same.
template <bool WIDE = false>
__device__ __forceinline__ void ppo_backward(const PolicyNet &net, const float *w, float *g, float *out, int tid, float *base = nullptr, float *top = nullptr,
                                             const float *park = nullptr)
{
    const int lane = tid & 63, wave = tid >> 6, q = lane >> 4, c = lane & 15;
    float *dz = out;
    if constexpr (WIDE) park += ppo_wide_scratch_floats(net);
    for (int l = net.n_layers - 1; l >= 0; l--) {
        const int K = net.kp[l], N = net.np[l], ldi = net_ld(K), ldo = net_ld(N), kb = K >> 4;
        float *a = dz - NET_ROWS * ldi;
        if constexpr (WIDE) {
            a = ppo_wide_buf(net, l, base, top);
            park -= NET_ROWS * ldi;
            ppo_copy_rows(a, park, K, tid);
            __syncthreads();
        }
        float *gW = g + net.w_off[l], *gb = g + net.b_off[l];
        for (int blk = wave; blk < (N >> 4) * kb; blk += 4) {
            const int nb = blk / kb, n0 = nb << 4, k0 = (blk - nb * kb) << 4;
            f32x4 acc = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int j = 0; j < 8; j++) {      // MFMA j: rows 4 j + q
                const int r = 4 * j + q;
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(dz[r * ldo + n0 + c], a[r * ldi + k0 + c], acc, 0, 0, 0);
            }
            // C/D map of the 16x16 block: column (k) = lane & 15, row (n) = 4 (lane >> 4) + register
#pragma unroll
            for (int i = 0; i < 4; i++) {
                float *p = gW + (size_t)(n0 + 4 * q + i) * K + k0 + c;
                *p = *p + acc[i];
            }
        }
        for (int n = tid; n < N; n += 256) {
            float s = 0.0f;
#pragma unroll 4
            for (int r = 0; r < NET_ROWS; r++) s += dz[r * ldo + n];
            gb[n] = gb[n] + s;
        }
        if (l == 0) break;
        __syncthreads();                       // (dW has read A: dZ' may overwrite it)
        const float *W = w + net.w_off[l];
        for (int blk = wave; blk < kb; blk += 4) {
            const int k0 = blk << 4;
            f32x4 acc[2] = {f32x4{0.0f, 0.0f, 0.0f, 0.0f}, f32x4{0.0f, 0.0f, 0.0f, 0.0f}};
            for (int n0 = 0; n0 < N; n0 += 16) {      // MFMA j: n = n0 + 4 q + j, the same permutation on both operands
                const float4 d0 = *(const float4 *)(dz + c * ldo + n0 + 4 * q), d1 = *(const float4 *)(dz + (16 + c) * ldo + n0 + 4 * q);
                const float *wp = W + (size_t)(n0 + 4 * q) * K + k0 + c;
                const float wv[4] = {wp[0], wp[K], wp[2 * K], wp[3 * K]};
                const float dv[2][4] = {{d0.x, d0.y, d0.z, d0.w}, {d1.x, d1.y, d1.z, d1.w}};
#pragma unroll
                for (int j = 0; j < 4; j++)
#pragma unroll
                    for (int mi = 0; mi < 2; mi++) acc[mi] = __builtin_amdgcn_mfma_f32_16x16x4f32(dv[mi][j], wv[j], acc[mi], 0, 0, 0);
            }
#pragma unroll
            for (int mi = 0; mi < 2; mi++)
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    float *p = a + (mi * 16 + 4 * q + i) * ldi + k0 + c;
                    const float av = *p;
                    *p = acc[mi][i] * (net.act == RANENV_ACT_RELU ? (av > 0.0f ? 1.0f : 0.0f) : 1.0f - av * av);
                }
        }
        __syncthreads();
        dz = a;
    }
}

// The sum of the workgroup's 256 partial sums, in slot order, in every thread (two barriers: the slots are free again on return)
__device__ __forceinline__ double ppo_sum(double *red, double part, int tid)
{
    red[tid] = part;
    __syncthreads();
    double tot = 0.0;
#pragma unroll 1
    for (int k = 0; k < 256; k++) tot += red[k];
    __syncthreads();
    return tot;
}

__device__ __forceinline__ void ppo_adam(float *w, float *m, float *v, const float *g, long long n, float scale, float b1, float omb1, float b2, float omb2,
                                         float step, float sbc2, float eps, int tid)
{
#pragma unroll 1
    for (long long i = tid; i < n; i += 256) {
        const float gi = g[i] * scale;
        const float mi = b1 * m[i] + omb1 * gi;
        const float vi = b2 * v[i] + (omb2 * gi) * gi;
        m[i] = mi; v[i] = vi;
        w[i] = w[i] - step * (mi / (sqrtf(vi) / sbc2 + eps));
    }
}

// b^t (t >= 1) in float64 by repeated squaring
__device__ __forceinline__ double ppo_powi(double b, int t)
{
    double r = 1.0;
#pragma unroll 1
    for (; t > 0; t >>= 1) { if (t & 1) r *= b; b *= b; }
    return r;
}

}  // namespace
