// ranenv_ppo_parts.hpp -- the one statement of every step the training kernels share (ranenv_ppo.hip: the PPO updates of the bound nets
// and of the head policies; ranenv_ppo_spread.hip: one agent's PPO update spread over the chip, the IBSched pair's and the head pair's
// -- whose elementwise reduce / apply steps (ppo_spread_*) stand at the end; ranenv_sac.hip: the SAC update): the LDS size of a net's
// rows, the backward pass of one 32-row tile on the f32 matrix cores and its dZ' block walk (ppo_backward_bf16: a bf16 net's, on the
// bf16 matrix cores, with ppo_bf16_reround, which keeps its acting copies at bf16 of the master), the workgroup sum in slot order, Adam's
// constants and float32 element step, and the steps of a PPO minibatch -- zeroing, the advantages' mean and std, the tile's row list,
// the clipped surrogate, the critic row, the joint norm and clip scale, the statistics, the gradient copy -- and the 32-row tile
// itself, once per pair of nets: ppo_tile for the IBSched nets (the member update and the spread pass; its steps: the record cell, the
// input rows, the wide forward pass, the actor's row) and ppo_head_tile for the head pair (ppo_head_load_rows, ppo_head_actor_tile).
// A rule that lives here (the weight-read rule at ppo_tile, the tiles' barriers, the 1e-6 of the clip, the 1e-8 of the std, the tie
// rule of torch.minimum, Adam's operation order) has no second text.  ranenv_ppo.hip's header comment describes the plan they belong to.
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

// Bytes of LDS for the rows of a bf16 net (ranenv_ppo_bind_spread_bfloat): the input's and every hidden layer's 32 rows in bf16 at stride
// net_ld16, the output layer's in f32 at stride net_ld -- net_layers<true, true>'s layout
__host__ __device__ inline int ppo_bf16_act_bytes(const PolicyNet &net)
{
    int n = 0;
    for (int l = 0; l < net.n_layers; l++) n += NET_ROWS * net_ld16(net.kp[l]) * 2;
    return n + NET_ROWS * net_ld(net.np[net.n_layers - 1]) * 4;
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

// dZ'[r][k] = (sum_n dZ[r][n] W[n][k]) act'(A[r][k]) for the 16-column blocks [b0, b1) of layer l's input rows `a`, written in place
// over them (the activation's derivative is taken from its value; layer 0's "activation" is the input: factor 1).  `W` = layer l's
// weights, `dz` its output rows' gradient.  No barrier: the caller holds one in front (whoever read A is done) and one behind.
// The empty asm makes the four W values of a step live at one point, so their loads are in flight together and the step waits once.
// Left to itself the register allocator gave the four one register in some kernels (a wait per load) and two in others, by what else
// the kernel held: the walk's time then moved by a few per cent, up or down, with any edit of a caller.
__device__ __forceinline__ void ppo_dz_blocks(const PolicyNet &net, int l, const float *W, const float *dz, float *a, int b0, int b1, int tid)
{
    const int lane = tid & 63, wave = tid >> 6, q = lane >> 4, c = lane & 15;
    const int K = net.kp[l], N = net.np[l], ldi = net_ld(K), ldo = net_ld(N);
    for (int blk = b0 + wave; blk < b1; blk += 4) {
        const int k0 = blk << 4;
        f32x4 acc[2] = {f32x4{0.0f, 0.0f, 0.0f, 0.0f}, f32x4{0.0f, 0.0f, 0.0f, 0.0f}};
        for (int n0 = 0; n0 < N; n0 += 16) {      // MFMA j: n = n0 + 4 q + j, the same permutation on both operands
            const float4 d0 = *(const float4 *)(dz + c * ldo + n0 + 4 * q), d1 = *(const float4 *)(dz + (16 + c) * ldo + n0 + 4 * q);
            const float *wp = W + (size_t)(n0 + 4 * q) * K + k0 + c;
            const float wv[4] = {wp[0], wp[K], wp[2 * K], wp[3 * K]};
            asm volatile("" ::"v"(wv[0]), "v"(wv[1]), "v"(wv[2]), "v"(wv[3]));
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
                *p = acc[mi][i] * (l == 0 ? 1.0f : (net.act == RANENV_ACT_RELU ? (av > 0.0f ? 1.0f : 0.0f) : 1.0f - av * av));
            }
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
        ppo_dz_blocks(net, l, w + net.w_off[l], dz, a, 0, kb, tid);
        __syncthreads();
        dz = a;
    }
}

// The backward pass of one tile of a bf16 net (ranenv_ppo_bind_spread_bfloat; include/ranenv.h states the contract) on the bf16 matrix
// cores: `out` = the output layer's f32 rows, holding G = dL/d(output); in front of them the bf16 rows of every layer's input, as
// net_layers<true, true> left them.  D_L = bf16(G) is written over G first (a bf16 row lies below the f32 row it comes from, so chunks
// of 256 elements in ascending order, each read in front of a barrier and written behind it, never overwrite a value still to be read).
// Layer l: dW_l = D_l^T A_{l-1} -- the tile's 32 rows are ONE MFMA's K, a 16x16 block of dW is one MFMA; both operands are column
// reads of the row-major rows (16-bit LDS reads) --, db_l the column sums of D_l, both added in f32 into `g` (the F32 packed layout:
// bf.w_off / b_off); then D_{l-1} = bf16((D_l Wq_l) act'(A_{l-1})) over A_{l-1} in place: D_l by rows from LDS, Wq_l from the
// transposed copy bf.wt (Wt [kp][np]: a 16-byte load per lane and 32 n, a vector load at a lane-dependent address -- THE WEIGHT-READ
// RULE at ppo_tile holds for both bf16 copies), act' from the rounded activation.  Dead rows are zero rows of G.  Ends without a barrier.
__device__ __forceinline__ void ppo_backward_bf16(const PolicyNet &net, const PpoBf16Net &bf, float *g, float *out, int tid)
{
    const int lane = tid & 63, wave = tid >> 6, q = lane >> 4, c = lane & 15;
    const int L = net.n_layers;
    {
        const int N = net.np[L - 1], ldf = net_ld(N), ldo = net_ld16(N);
        __bf16 *d = (__bf16 *)out;
        for (int e0 = 0; e0 < NET_ROWS * N; e0 += 256) {
            const int e = e0 + tid, r = e / N, n = e - r * N;
            const float v = out[r * ldf + n];
            __syncthreads();
            d[r * ldo + n] = (__bf16)v;
        }
        __syncthreads();
    }
    __bf16 *dz = (__bf16 *)out;
    for (int l = L - 1; l >= 0; l--) {
        const int K = net.kp[l], N = net.np[l], ldi = net_ld16(K), ldo = net_ld16(N), kb = K >> 4;
        __bf16 *a = dz - NET_ROWS * ldi;
        float *gW = g + bf.w_off[l], *gb = g + bf.b_off[l];
        for (int blk = wave; blk < (N >> 4) * kb; blk += 4) {
            const int nb = blk / kb, n0 = nb << 4, k0 = (blk - nb * kb) << 4;
            bf16x8 dv, av;                     // operand element j: tile row 8 q + j
#pragma unroll
            for (int j = 0; j < 8; j++) { dv[j] = dz[(8 * q + j) * ldo + n0 + c]; av[j] = a[(8 * q + j) * ldi + k0 + c]; }
            const f32x4 acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dv, av, f32x4{0.0f, 0.0f, 0.0f, 0.0f}, 0, 0, 0);
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
            for (int r = 0; r < NET_ROWS; r++) s += (float)dz[r * ldo + n];
            gb[n] = gb[n] + s;
        }
        if (l == 0) break;
        __syncthreads();                       // (dW has read A: D' may overwrite it)
        const __bf16 *Wt = (const __bf16 *)(bf.wt + net.w_off[l]);
        for (int blk = wave; blk < kb; blk += 4) {
            const int k0 = blk << 4;
            f32x4 acc[2] = {f32x4{0.0f, 0.0f, 0.0f, 0.0f}, f32x4{0.0f, 0.0f, 0.0f, 0.0f}};
            const bf16x8 *wp = (const bf16x8 *)(Wt + (size_t)(k0 + c) * N) + q;      // MFMA k: n = n0 + 8 q .. + 7 on both operands
            const __bf16 *d0 = dz + c * ldo + 8 * q, *d1 = dz + (16 + c) * ldo + 8 * q;
            bf16x8 b = wp[0];
            for (int n0 = 0; n0 < N; n0 += 32) {
                const bf16x8 nb = wp[(n0 + 32 < N ? n0 + 32 : n0) >> 3];
                acc[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8 *)(d0 + n0), b, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*(const bf16x8 *)(d1 + n0), b, acc[1], 0, 0, 0);
                b = nb;
            }
#pragma unroll
            for (int mi = 0; mi < 2; mi++)
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    __bf16 *p = a + (mi * 16 + 4 * q + i) * ldi + k0 + c;
                    const float av = (float)*p;
                    *p = (__bf16)(acc[mi][i] * (net.act == RANENV_ACT_RELU ? (av > 0.0f ? 1.0f : 0.0f) : 1.0f - av * av));
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

// b^t (t >= 1) in float64 by repeated squaring
__device__ __forceinline__ double ppo_powi(double b, int t)
{
    double r = 1.0;
#pragma unroll 1
    for (; t > 0; t >>= 1) { if (t & 1) r *= b; b *= b; }
    return r;
}

// Adam at step t (>= 1): the constants in float64, rounded once -- step = lr / (1 - b1^t), sbc2 = sqrt(1 - b2^t) -- and the float32
// element step on an already scaled gradient g, torch's operation order: m, v, then w - step * (m / (sqrt(v) / sbc2 + eps))
struct AdamStep { float b1, omb1, b2, omb2, eps, step, sbc2; };
__device__ __forceinline__ AdamStep adam_step(double lr, double beta1, double beta2, double eps, int t)
{
    return AdamStep{(float)beta1, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps,
                    (float)(lr / (1.0 - ppo_powi(beta1, t))), (float)sqrt(1.0 - ppo_powi(beta2, t))};
}
__device__ __forceinline__ void adam_elem(float &w, float &m, float &v, float g, const AdamStep &a)
{
    const float mi = a.b1 * m + a.omb1 * g;
    const float vi = a.b2 * v + (a.omb2 * g) * g;
    m = mi; v = vi;
    w = w - a.step * (mi / (sqrtf(vi) / a.sbc2 + a.eps));
}
__device__ __forceinline__ void ppo_adam(float *w, float *m, float *v, const float *g, long long n, float scale, const AdamStep &a, int tid)
{
#pragma unroll 1
    for (long long i = tid; i < n; i += 256) adam_elem(w[i], m[i], v[i], g[i] * scale, a);
}

// ---- the steps of a PPO minibatch (ppo_update_body and ranenv_ppo_update_kernel_head, ranenv_ppo.hip) -------------------------------------
__device__ __forceinline__ void ppo_zero(float *g, long long floats, int tid)
{
#pragma unroll 1
    for (long long i = tid; i < floats; i += 256) g[i] = 0.0f;
}

// The minibatch's advantage mean and std + 1e-8 (torch's unbiased std; one row: 0): two float64 passes over adv_at(k), k < nb -- the
// caller's cell of list entry k, 0.0 for an entry outside the record
template <class F>
__device__ __forceinline__ void ppo_adv_norm(double *red, int nb, int tid, F adv_at, double &a_mean, double &a_den)
{
    double s = 0.0;
#pragma unroll 1
    for (int k = tid; k < nb; k += 256) s += adv_at(k);
    a_mean = ppo_sum(red, s, tid) / (double)nb;
    s = 0.0;
#pragma unroll 1
    for (int k = tid; k < nb; k += 256) { const double d = adv_at(k) - a_mean; s += d * d; }
    const double ss = ppo_sum(red, s, tid);
    a_den = (nb > 1 ? sqrt(ss / (double)(nb - 1)) : 0.0) + 1e-8;
}

// The tile's record rows: rowidx[r] = entry c0 + t0 + r of `list`, or -1 beyond the minibatch's nb entries and outside the record
__device__ __forceinline__ void ppo_list_rows(int *rowidx, const int32_t *list, int c0, int t0, int nb, long long n_record, int tid)
{
    if (tid >= NET_ROWS) return;
    int i = -1;
    if (t0 + tid < nb) { i = list[c0 + t0 + tid]; if (i < 0 || i >= n_record) i = -1; }
    rowidx[tid] = i;
}

// The clipped surrogate of one live row: rs[0..4] = policy loss, entropy (the caller's `ent`), logp_old - logp, clipped?, live;
// returns gl = dL/d(logp) of the row.  torch.minimum / clamp: the unclipped branch carries the gradient where it is the smaller one,
// both where they tie
__device__ __forceinline__ double ppo_surrogate(double lp, double lp_old, double adv, double ent, double clip, double wrow, double *rs)
{
    const double ratio = exp(lp - lp_old), c_lo = 1.0 - clip, c_hi = 1.0 + clip;
    const bool inside = ratio >= c_lo && ratio <= c_hi;
    const double s1 = ratio * adv, s2 = (ratio < c_lo ? c_lo : (ratio > c_hi ? c_hi : ratio)) * adv;
    const double dsdr = inside || s1 < s2 ? adv : 0.0;
    rs[0] = -(s1 < s2 ? s1 : s2); rs[1] = ent; rs[2] = lp_old - lp; rs[3] = inside ? 0.0 : 1.0; rs[4] = 1.0;
    return -(dsdr * ratio) * wrow;
}

// The critic's row i (< 0: dead): o[0] = V becomes dL/dV = 2 vf_coeff (V - vtarg) / rows; returns the squared error.  vtarg_at():
// the row's target, read for a live row alone
template <class F>
__device__ __forceinline__ double ppo_critic_row(float *o, int i, F vtarg_at, double vf_coeff, double wrow)
{
    if (i < 0) { o[0] = 0.0f; return 0.0; }
    const double d = (double)o[0] - (double)vtarg_at();
    o[0] = (float)(((2.0 * d) * vf_coeff) * wrow);
    return d * d;
}

// Thread 0's statistics of an epoch; a tile's rows 0..31 added in order from their `stride` doubles each (ppo_surrogate's five, then
// the value loss where `critic`), and the epoch's eight outputs over its n rows
struct PpoEpoch { double pl = 0.0, vl = 0.0, ent = 0.0, kl = 0.0, cf = 0.0, gn = 0.0, rows = 0.0; int n_mb = 0; };
__device__ __forceinline__ void ppo_tile_stats(PpoEpoch &st, const double *rowstat, int stride, bool critic)
{
#pragma unroll 1
    for (int r = 0; r < NET_ROWS; r++) {
        const double *rs = rowstat + r * stride;
        st.pl += rs[0]; st.ent += rs[1]; st.kl += rs[2]; st.cf += rs[3]; st.rows += rs[4];
        if (critic) st.vl += rs[5];
    }
}
__device__ __forceinline__ void ppo_epoch_stats(double *out, const PpoEpoch &st, int n)
{
    const double inv = 1.0 / (double)n;
    out[0] = st.pl * inv; out[1] = st.vl * inv; out[2] = st.ent * inv; out[3] = st.kl * inv; out[4] = st.cf * inv; out[5] = st.gn * inv;
    out[6] = st.rows; out[7] = (double)st.n_mb;
}

// The thread's share of a gradient tensor's sum of squares, added to `s` element by element: the nets of a minibatch continue ONE
// accumulator, so the joint norm's summation order does not depend on where a tensor ends
__device__ __forceinline__ double ppo_sq_sum(const float *g, long long floats, int tid, double s)
{
#pragma unroll 1
    for (long long i = tid; i < floats; i += 256) { const double x = (double)g[i]; s += x * x; }
    return s;
}

// torch's clip_grad_norm_ factor for the joint norm (grad_clip <= 0: no clip)
__device__ __forceinline__ double ppo_clip_scale(double grad_clip, double norm)
{
    if (!(grad_clip > 0.0)) return 1.0;
    const double sc = grad_clip / (norm + 1e-6);
    return sc < 1.0 ? sc : 1.0;
}

__device__ __forceinline__ void ppo_grad_out(float *out, const float *g, long long floats, int tid)
{
#pragma unroll 1
    for (long long i = tid; i < floats; i += 256) out[i] = g[i];
}

// ---- the tile of the IBSched nets and its steps (ppo_update_body, ranenv_ppo.hip, and the spread pass, ranenv_ppo_spread.hip) ----------
constexpr int PPO_FIXED = 4096;           // bytes of LDS in front of the rows: reduction slots, per-row statistics, the tile's record rows
constexpr int PPO_ROW_STATS = 6;          // per row: policy loss, entropy, logp_old - logp, clipped?, live?, value loss

// The (logp, adv, vtarg) cell of record row i: column 0 of the inter row, column s + 1 of the env's row for slice s
__device__ __forceinline__ size_t ppo_cell(int kind, int i, int S) { return kind == 0 ? (size_t)i * (S + 1) : (size_t)(i / S) * (S + 1) + 1 + (i % S); }

// The tile's rows of `net`'s input -> buffer 0: row r is record row idx[r] (< 0: a dead row, zeros), read as net_load_rows reads an
// env's row -- the inter observation, or the slice's observation behind, for RANENV_NET_IN_MASK_OBS, its mask as floats.  BF: a bf16
// net's rows, rounded to bf16 at stride net_ld16 (load_rows)
template <bool BF = false>
__device__ __forceinline__ void ppo_load_rows(const PolicyNet &net, const PpoArgs &A, int kind, const int *idx, float *dst, int tid)
{
    load_rows<BF>(net.kp[0], 0, 0, dst, tid, [&](int r, int k) {
        const int i = idx[r];
        if (i < 0 || k >= net.in_dim) return 0.0f;
        if (kind == 0) return A.traj.obs_inter[(size_t)i * (size_t)(10 * A.S) + k];
        const int ko = net.layout == RANENV_NET_IN_MASK_OBS ? k - A.Us : k;
        if (ko < 0) return (float)A.traj.mask_intra[(size_t)i * A.Us + k];
        return A.traj.obs_intra[(size_t)i * A.W + ko];
    });
}

// The forward pass of one tile on the two buffers: the input rows lie at `base` behind a barrier.  Layer l parks its input rows in
// slab l of `park` while it reads them (the barrier in front published them; nothing overwrites them before the layer's own barrier)
// and writes the other buffer.  Returns the output layer's rows.
__device__ __forceinline__ float *ppo_forward_wide(const PolicyNet &net, const float *w, float *base, float *top, float *park, int tid)
{
    float *in = base;
    for (int l = 0; l < net.n_layers; l++) {
        float *out = ppo_wide_buf(net, l + 1, base, top);
        ppo_copy_rows(park, in, net.kp[l], tid);
        net_layer_f32(net, l, w, in, out, tid & 63, tid >> 6);
        __syncthreads();
        park += NET_ROWS * net_ld(net.kp[l]);
        in = out;
    }
    return in;
}

// The loss gradient at the actor's outputs for the tile's row r (thread r): `o` = the row's outputs, overwritten; the row's statistics
__device__ __forceinline__ void ppo_actor_row(const PpoArgs &A, const ranenv_ppo_hparams &hp, int kind, int i, int np, float *o, double *rs, double wrow,
                                              double a_mean, double a_den)
{
    const int S = A.S;
    if (i < 0) {
#pragma unroll 1
        for (int j = 0; j < np; j++) o[j] = 0.0f;
        rs[0] = rs[1] = rs[2] = rs[3] = rs[4] = 0.0;
        return;
    }
    const size_t at = ppo_cell(kind, i, S);
    const double lp_old = (double)A.traj.logp[at];
    const double adv = hp.adv_norm ? ((double)A.traj.adv[at] - a_mean) / a_den : (double)A.traj.adv[at];
    double lp = 0.0, ent = 0.0;
    int j0 = 0, ch = 0;
    double p0 = 0.0, p1 = 0.0, p2 = 0.0, q0 = 0.0, q1 = 0.0, q2 = 0.0;
    if (kind == 0) {
        int n_act = 0;
#pragma unroll 1
        for (int s = 0; s < S; s++) n_act += A.traj.mask_inter[(size_t)i * S + s] != 0 ? 1 : 0;
        j0 = S - n_act;
#pragma unroll 1
        for (int j = j0; j < S; j++) {
            const double ls = (double)o[S + j];
            const double z = (A.traj.action_inter[(size_t)i * S + j] - (double)o[j]) / exp(ls);
            lp += RANENV_INTER_LOGP_TERM(z, ls);
            ent += (ls + 0.5) + HALF_LN_2PI;
        }
        lp += RANENV_INTER_LOGP_MASKED(j0);
    } else {
        const float l0 = o[0], l1 = o[1], l2 = o[2];
        ch = (int)A.traj.action_intra[i];
        // (RANENV_INTRA_LOGP's expressions in its order, for all three logits: change the two together, ranenv_net.hpp)
        const double mx = fmax(fmax((double)l0, (double)l1), (double)l2);
        const double e0 = exp((double)l0 - mx), e1 = exp((double)l1 - mx), e2 = exp((double)l2 - mx);
        const double sum = (e0 + e1) + e2, lsum = log(sum);
        q0 = ((double)l0 - mx) - lsum; q1 = ((double)l1 - mx) - lsum; q2 = ((double)l2 - mx) - lsum;
        p0 = e0 / sum; p1 = e1 / sum; p2 = e2 / sum;
        lp = ch == 0 ? q0 : (ch == 1 ? q1 : q2);
        ent = -((p0 * q0 + p1 * q1) + p2 * q2);
    }
    if (A.probe_logp) A.probe_logp[at] = (float)lp;
    const double gl = ppo_surrogate(lp, lp_old, adv, ent, hp.clip, wrow, rs), ge = hp.ent_coeff * wrow;
    if (kind == 0) {
#pragma unroll 1
        for (int j = 0; j < j0; j++) { o[j] = 0.0f; o[S + j] = 0.0f; }
#pragma unroll 1
        for (int j = j0; j < S; j++) {
            const double sig = exp((double)o[S + j]);
            const double z = (A.traj.action_inter[(size_t)i * S + j] - (double)o[j]) / sig;
            o[j] = (float)(gl * (z / sig));
            o[S + j] = (float)(gl * (z * z - 1.0) - ge);
        }
    } else {
        o[0] = (float)(gl * ((ch == 0 ? 1.0 : 0.0) - p0) + ge * (p0 * (q0 + ent)));
        o[1] = (float)(gl * ((ch == 1 ? 1.0 : 0.0) - p1) + ge * (p1 * (q1 + ent)));
        o[2] = (float)(gl * ((ch == 2 ? 1.0 : 0.0) - p2) + ge * (p2 * (q2 + ent)));
    }
}

// One 32-row tile of a minibatch, entries c0 + t0 .. of `list`: the rows are listed, then per net (0 the actor, 1 the critic) loaded,
// run forward, turned into dL/d(output) and run backward, and thread 0 adds the rows' statistics to `st`.  The callers differ in where
// net k's descriptor lies (net_at(k) -> const PolicyNet &: the kernel argument, or the member's copy in LDS), where its weights are
// (w_at(k)) and where its gradient goes (g_at(k): the member's block, or the workgroup's slab).  WIDE: on the workgroup's parked rows
// `wpark`.  THE WEIGHT-READ RULE of the training kernels stands here and at ppo_head_tile: the weights are what the launch itself, or
// the launch before, wrote by vector stores, so every weight read -- the forward's float4 and bias loads, the backward's W loads -- is
// a vector load at a lane-dependent address behind a workgroup barrier, never a read through the scalar cache; log_std is read through
// its LDS copy.  Ends without a barrier: the next tile's first, or the caller's, is the one behind the backward pass.
// BF (ranenv_ppo_bind_spread_bfloat; never WIDE): the nets are bf16 ones -- net_at(k) the acting copy's layout, w_at(k) that copy, on which
// the forward pass is the acting kernels' (net_layers<true>: the re-evaluated log-probability is the recorded one while the weights
// stand), bf[k] the f32 layout's offsets and the transposed copy for ppo_backward_bf16, g_at(k) in the f32 layout.
template <bool WIDE, bool BF = false, class NetAt, class WAt, class GAt>
__device__ __forceinline__ void ppo_tile(const PpoArgs &A, const ranenv_ppo_hparams &hp, int kind, int n_nets, const int32_t *list, int c0, int t0, int nb,
                                         long long n_record, double wrow, double a_mean, double a_den, double *rowstat, int *rowidx, float *act, float *wpark,
                                         PpoEpoch &st, int tid, NetAt net_at, WAt w_at, GAt g_at, const PpoBf16Net *bf = nullptr)
{
    static_assert(!(WIDE && BF), "bf16 rows fit the LDS plan where the wide plan was needed");
    const int lane = tid & 63, wave = tid >> 6, S = A.S;
    __syncthreads();                           // (the previous tile's backward pass and statistics are read)
    ppo_list_rows(rowidx, list, c0, t0, nb, n_record, tid);
    // ---- per net: forward, dL/d(output) per row, backward ---------------------------------------------------------------------------
#pragma unroll 1
    for (int k = 0; k < n_nets; k++) {
        const PolicyNet &net = net_at(k);
        const float *w = w_at(k);
        float *g = g_at(k);
        __syncthreads();                       // (the tile's rows are listed; the actor's backward pass has read its rows)
        float *cur = act, *nxt = act + NET_ROWS * (BF ? net_ld16(net.kp[0]) / 2 : net_ld(net.kp[0]));
        ppo_load_rows<BF>(net, A, kind, rowidx, cur, tid);
        __syncthreads();
        if constexpr (WIDE) cur = ppo_forward_wide(net, w, act, act + ppo_wide_floats(net), wpark, tid);
        else net_layers<BF, true>(net, w, cur, nxt, lane, wave);
        if (tid < NET_ROWS) {
            const int i = rowidx[tid], np = net.np[net.n_layers - 1];
            float *o = cur + tid * net_ld(np);
            double *rs = rowstat + tid * PPO_ROW_STATS;
            if (k == 0) ppo_actor_row(A, hp, kind, i, np, o, rs, wrow, a_mean, a_den);
            else rs[5] = ppo_critic_row(o, i, [&] { return A.traj.vtarg[ppo_cell(kind, i, S)]; }, hp.vf_coeff, wrow);
        }
        __syncthreads();
        if constexpr (BF) ppo_backward_bf16(net, bf[k], g, cur, tid);
        else if constexpr (WIDE) ppo_backward<true>(net, w, g, cur, tid, act, act + ppo_wide_floats(net), wpark);
        else ppo_backward(net, w, g, cur, tid);
    }
    if (tid == 0) ppo_tile_stats(st, rowstat, PPO_ROW_STATS, n_nets == 2);      // (the barriers above have published the rows')
}

// ---- the tile of the head policies and its steps (ranenv_ppo_update_kernel_head and the spread head pass, ranenv_ppo_spread.hip) ------
constexpr int PPO_HEAD_ROW_STATS = 7;     // PPO_ROW_STATS' six, then gl = dL/d(logp) of the row
static_assert(PPO_FIXED >= (256 + NET_ROWS * PPO_HEAD_ROW_STATS) * 8 + NET_ROWS * 4 + 16 * 4, "the fixed LDS region holds the head kernels' row statistics and log_std");

__device__ __forceinline__ void ppo_head_load_rows(const PolicyNet &net, const PpoHeadArgs &A, const int *idx, float *dst, int tid)
{
    load_rows(net.kp[0], 0, 0, dst, tid, [&](int r, int k) {
        const int i = idx[r];
        if (i < 0 || k >= net.in_dim) return 0.0f;
        return A.traj.obs_head[(size_t)i * (size_t)(10 * A.S) + k];
    });
}

// The loss gradient at the head actor's outputs for one tile, three steps with a barrier between them (the caller holds one in front
// -- the forward pass has written `cur` -- and one behind): `cur` = the output rows at stride `ldo`, overwritten; `lsw` = log_std [S]
// and `sig` = exp(log_std) in float64, both in LDS; rowstat[r][0..4], [6] = the row's statistics and gl; thread j < S adds the tile's
// d/d log_std_j to its `g_ls`, rows in ascending order.
__device__ __forceinline__ void ppo_head_actor_tile(const PpoHeadArgs &A, const int *rowidx, float *cur, int np, int ldo, double *rowstat, const float *lsw,
                                                    const double *sig, double wrow, double a_mean, double a_den, double &g_ls, int tid)
{
    const ranenv_ppo_hparams &hp = A.hp;
    const int S = A.S;
    const double ge = hp.ent_coeff * wrow;
    // 1. the row's log-probability, ratio and statistics (thread r); the outputs stay
    if (tid < NET_ROWS) {
        const int i = rowidx[tid];
        const float *o = cur + tid * ldo;
        double *rs = rowstat + tid * PPO_HEAD_ROW_STATS;
        if (i < 0) rs[0] = rs[1] = rs[2] = rs[3] = rs[4] = rs[6] = 0.0;
        else {
            const double lp_old = (double)A.traj.logp[i];
            const double adv = hp.adv_norm ? ((double)A.traj.adv[i] - a_mean) / a_den : (double)A.traj.adv[i];
            double lp = 0.0, ent = 0.0;
#pragma unroll 1
            for (int j = 0; j < S; j++) {
                const double ls = (double)lsw[j];
                const double z = (A.traj.action[(size_t)i * S + j] - (double)o[j]) / sig[j];
                lp += RANENV_INTER_LOGP_TERM(z, ls);
                ent += (ls + 0.5) + HALF_LN_2PI;
            }
            rs[6] = ppo_surrogate(lp, lp_old, adv, ent, hp.clip, wrow, rs);
        }
    }
    __syncthreads();
    // 2. d/d log_std_j (thread j), rows in ascending order, float64
    if (tid < S) {
        const double sj = sig[tid];
#pragma unroll 1
        for (int r = 0; r < NET_ROWS; r++) {
            const int i = rowidx[r];
            if (i < 0) continue;
            const double z = (A.traj.action[(size_t)i * S + tid] - (double)cur[r * ldo + tid]) / sj;
            g_ls += rowstat[r * PPO_HEAD_ROW_STATS + 6] * (z * z - 1.0) - ge;
        }
    }
    __syncthreads();
    // 3. d/d mean_j over the outputs, element by element; dead rows and padded columns: zeros
#pragma unroll 1
    for (int e = tid; e < NET_ROWS * np; e += 256) {
        const int r = e / np, j = e - r * np, i = rowidx[r];
        float *o = cur + r * ldo + j;
        float v = 0.0f;
        if (i >= 0 && j < S) {
            const double sj = sig[j], z = (A.traj.action[(size_t)i * S + j] - (double)*o) / sj;
            v = (float)(rowstat[r * PPO_HEAD_ROW_STATS + 6] * (z / sj));
        }
        *o = v;
    }
}

// One 32-row tile of a minibatch of the head pair, ppo_tile's steps on the head record (its weight-read rule holds here): the actor's
// gradient at its outputs is ppo_head_actor_tile's, which adds to thread j's `g_ls`; g_at(k): where net k's gradient goes.
template <class GAt>
__device__ __forceinline__ void ppo_head_tile(const PpoHeadArgs &A, const int32_t *list, int c0, int t0, int nb, long long n_record, double wrow, double a_mean,
                                              double a_den, double *rowstat, int *rowidx, const float *lsw, const double *sig, float *act, double &g_ls,
                                              PpoEpoch &st, int tid, GAt g_at)
{
    const ranenv_ppo_hparams &hp = A.hp;
    const int lane = tid & 63, wave = tid >> 6;
    __syncthreads();                           // (the previous tile's backward pass and statistics are read)
    ppo_list_rows(rowidx, list, c0, t0, nb, n_record, tid);
#pragma unroll 1
    for (int k = 0; k < 2; k++) {
        const PpoNet &pn = A.net[k];
        const PolicyNet &net = pn.net;
        __syncthreads();                       // (the tile's rows are listed; the actor's backward pass has read its rows)
        float *cur = act, *nxt = act + NET_ROWS * net_ld(net.kp[0]);
        ppo_head_load_rows(net, A, rowidx, cur, tid);
        __syncthreads();
        net_layers<false, true>(net, pn.w, cur, nxt, lane, wave);
        const int np = net.np[net.n_layers - 1], ldo = net_ld(np);
        if (k == 1) {
            if (tid < NET_ROWS) {
                const int i = rowidx[tid];
                rowstat[tid * PPO_HEAD_ROW_STATS + 5] = ppo_critic_row(cur + tid * ldo, i, [&] { return A.traj.vtarg[i]; }, hp.vf_coeff, wrow);
            }
        } else ppo_head_actor_tile(A, rowidx, cur, np, ldo, rowstat, lsw, sig, wrow, a_mean, a_den, g_ls, tid);
        __syncthreads();
        ppo_backward(net, pn.w, g_at(k), cur, tid);
    }
    if (tid == 0) ppo_tile_stats(st, rowstat, PPO_HEAD_ROW_STATS, true);      // (the barriers above have published the rows')
}

// ---- the elementwise steps of a spread update (ranenv_ppo_spread.hip: the IBSched kinds' and the head pair's reduce and apply) --------
// Element e of the packed floats the launch covers: the four arrays' cells -- the actor's (n0) below its floats `af`, the critic's behind
struct PpoSpreadCell { float *g, *w, *m, *v; };
__device__ __forceinline__ PpoSpreadCell ppo_spread_cell(const PpoNet &n0, const PpoNet &n1, long long af, long long e)
{
    return e < af ? PpoSpreadCell{n0.g + e, n0.w + e, n0.m + e, n0.v + e} : PpoSpreadCell{n1.g + (e - af), n1.w + (e - af), n1.m + (e - af), n1.v + (e - af)};
}

// The reduce of the block's PPO_SPREAD_BLOCK elements: g[e] = the `used` slabs' [e] summed in ascending slab order, the cells zeroed
// for the next step; returns the thread's float64 share of the block's sum of squares
template <class F>
__device__ __forceinline__ double ppo_spread_reduce_elems(float *slab, long long slab_stride, int used, long long floats, int tid, F cell_at)
{
    double s = 0.0;
#pragma unroll 1
    for (int j = 0; j < PPO_SPREAD_BLOCK / 256; j++) {
        const long long e = (long long)blockIdx.x * PPO_SPREAD_BLOCK + j * 256 + tid;
        if (e >= floats) break;
        float *p = slab + e;
        float g = *p;
        *p = 0.0f;
#pragma unroll 1
        for (int u = 1; u < used; u++) {
            p += slab_stride;
            g = g + *p;
            *p = 0.0f;
        }
        *cell_at(e).g = g;
        s += (double)g * (double)g;
    }
    return s;
}

// The joint norm's square: ALL block partials in ascending order, in every thread of every block
__device__ __forceinline__ double ppo_spread_norm2(const double *bpart, int blocks)
{
    double tot = 0.0;
#pragma unroll 1
    for (int b = 0; b < blocks; b++) tot += bpart[b];
    return tot;
}

// The apply of the block's elements: Adam in place on the scaled gradient; `grad` (or null): the unclipped gradient's copy.
// stepped(e, w): what the bf16 binding does with element e's new value (ppo_bf16_reround)
template <class F, class R>
__device__ __forceinline__ void ppo_spread_apply_elems(long long floats, float *grad, float sc, const AdamStep &adam, int tid, F cell_at, R stepped)
{
#pragma unroll 1
    for (int j = 0; j < PPO_SPREAD_BLOCK / 256; j++) {
        const long long e = (long long)blockIdx.x * PPO_SPREAD_BLOCK + j * 256 + tid;
        if (e >= floats) break;
        const PpoSpreadCell c = cell_at(e);
        const float g = *c.g;
        if (grad) grad[e] = g;
        adam_elem(*c.w, *c.m, *c.v, g * sc, adam);
        stepped(e, *c.w);
    }
}
template <class F>
__device__ __forceinline__ void ppo_spread_apply_elems(long long floats, float *grad, float sc, const AdamStep &adam, int tid, F cell_at)
{
    ppo_spread_apply_elems(floats, grad, sc, adam, tid, cell_at, [](long long, float) {});
}

// Element x of a bf16 net's F32 packed layout has the value w (the master's, behind Adam or at the seed): a weight W_l[n][k] goes,
// rounded to nearest even, to the acting copy (bf16 [np][kp] at float net.w_off[l]) and to the transposed copy (Wt [kp][np] at the same
// float of bf.wt); a bias to the acting copy's f32 bias.  So acting == bf16(master) and Wt == acting^T behind every launch that calls it.
__device__ __forceinline__ void ppo_bf16_reround(const PolicyNet &net, const PpoBf16Net &bf, long long x, float w)
{
    for (int l = 0; l < net.n_layers; l++) {
        if (x < bf.b_off[l]) {
            const long long i = x - bf.w_off[l];
            const int K = net.kp[l], n = (int)(i / K), k = (int)(i - (long long)n * K);
            const __bf16 b = (__bf16)w;
            ((__bf16 *)(bf.acting + net.w_off[l]))[i] = b;
            ((__bf16 *)(bf.wt + net.w_off[l]))[(size_t)k * net.np[l] + n] = b;
            return;
        }
        if (x < bf.b_off[l] + net.np[l]) { bf.acting[net.b_off[l] + (x - bf.b_off[l])] = w; return; }
    }
}

// One thread's: a pass workgroup's row statistics of its tiles -> its PPO_SPREAD_STATS doubles of wstat, which ppo_spread_stats reads back
__device__ __forceinline__ void ppo_spread_wstat(double *out, const PpoEpoch &st)
{
    out[0] = st.pl; out[1] = st.ent; out[2] = st.kl; out[3] = st.cf; out[4] = st.rows; out[5] = st.vl;
}

// One thread's: the epoch's running sums `run` (PpoEpoch's fields in order) take this step's slab statistics wstat[0..geo.grid) in
// ascending order and the norm; the epoch's last step writes its eight outputs to `out`, every other one stores the sums back
__device__ __forceinline__ void ppo_spread_stats(double *run, const double *wstat, const PpoSpreadStep &geo, double norm, bool epoch_end, double *out, int n)
{
    PpoEpoch st;
    if (geo.mb > 0) { st.pl = run[0]; st.vl = run[1]; st.ent = run[2]; st.kl = run[3]; st.cf = run[4]; st.gn = run[5]; st.rows = run[6]; st.n_mb = (int)run[7]; }
#pragma unroll 1
    for (int u = 0; u < geo.grid; u++) {
        const double *ws = wstat + (size_t)u * PPO_SPREAD_STATS;
        st.pl += ws[0]; st.ent += ws[1]; st.kl += ws[2]; st.cf += ws[3]; st.rows += ws[4]; st.vl += ws[5];
    }
    st.gn += norm * (double)geo.nb;
    st.n_mb += 1;
    if (epoch_end) ppo_epoch_stats(out, st, n);
    else { run[0] = st.pl; run[1] = st.vl; run[2] = st.ent; run[3] = st.kl; run[4] = st.cf; run[5] = st.gn; run[6] = st.rows; run[7] = (double)st.n_mb; }
}

}  // namespace
