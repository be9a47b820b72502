// ranenv_net.hpp -- what the kernels that run the bound MLPs share (ranenv_policy.hip: the acting and recording launches;
// ranenv_ppo.hip: the PPO update; ranenv_sac.hip: the SAC update): the LDS row strides, the row loaders, the layers on the f32 / bf16 matrix cores and the
// float64 log-probability arithmetic of the IBSched distributions.  ranenv_policy.hip's header comment describes the decomposition.
#pragma once
#include "ranenv_numeric.hpp"
#include <type_traits>

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// LDS row stride in floats for a width x (a multiple of 32): = 4 mod 64, so that the 16 rows x 4 k of an operand load fall into
// distinct banks
__host__ __device__ inline int net_ld(int x) { return x + ((x & 63) ? 36 : 4); }

// ... and in bf16 elements for the rows of a bf16 net: 2 x + 32 bytes, an odd multiple of 32 mod 256 (2 x is a multiple of 64).  The
// LDS serves a 16-byte read in groups of 16 lanes that hold 16 distinct rows c, eight of them at k chunk q and eight at q + 1 (each
// eight distinct mod 8): row c then starts at 16-byte slot 2 (odd c) mod 16 of the 256-byte bank row -- the even slots once each for
// one chunk, the odd slots for the other -- so the 16 rows x 16 bytes of an operand read fall into distinct banks
__host__ __device__ inline int net_ld16(int x) { return x + 16; }

// Floats per row of an LDS buffer that holds any layer's input rows (BF: of a bf16 net) and the output layer's (f32) rows
template <bool BF = false>
__host__ __device__ inline int net_ld_max(const PolicyNet &net)
{
    int m = net_ld(net.np[net.n_layers - 1]);
    for (int l = 0; l < net.n_layers; l++) {
        const int ld = BF ? net_ld16(net.kp[l]) / 2 : net_ld(net.kp[l]);
        m = ld > m ? ld : m;
    }
    return m;
}

// The workgroup's 32 LDS rows of K0 columns at `dst` (stride net_ld(K0)) from at(row, column); columns [skip0, skip1) are left to the caller.
// BF: the rows of a bf16 net, rounded to nearest even (v_cvt_pk_bf16_f32), stride net_ld16(K0) bf16
template <bool BF = false, class F>
__device__ __forceinline__ void load_rows(int K0, int skip0, int skip1, float *dst, int tid, F at)
{
    const int ld0 = BF ? net_ld16(K0) : net_ld(K0);
    for (int i = tid; i < NET_ROWS * K0; i += 256) {
        const int r = i / K0, k = i - r * K0;
        if (k >= skip0 && k < skip1) continue;
        if constexpr (BF) ((__bf16 *)dst)[r * ld0 + k] = (__bf16)at(r, k);
        else dst[r * ld0 + k] = at(r, k);
    }
}

// Element (g, k) of the dense float array src [n][width], 0 beyond column `cols` and beyond row n.  `rec` non-null: a copy of the
// array in the making, the element is written there on the way.
__device__ __forceinline__ float dense_at(const float *src, float *rec, long long g, long long n, int width, int cols, int k)
{
    if (g >= n || k >= cols) return 0.0f;
    const size_t at = (size_t)g * (size_t)width + k;
    const float v = src[at];
    if (rec) rec[at] = v;
    return v;
}

// Rows first .. first + 31 of such an array -> LDS with zero padding
__device__ __forceinline__ void load_dense_rows(const float *src, long long first, long long n, int width, int cols, int K0, int skip0, int skip1, float *dst, int tid)
{
    load_rows(K0, skip0, skip1, dst, tid, [&](int r, int k) { return dense_at(src, nullptr, first + r, n, width, cols, k); });
}

// THE ROW MAP: which env `e` and slice `s` row g of a launch from env e0 on belongs to, and es = e * S + s, the row of the
// [B][S] arrays.  kind 0 (inter, head): row g = env e0 + g (s = 0).  kind 1 (intra): row g = e0 * S + g of the flat env x S rows, or
// -- SLICED, the workgroup's slice `sl` -- (env e0 + g, slice sl).  Every site of policy_body that addresses by row goes through here.
struct RowAt { int e, s; size_t es; };
template <bool SLICED>
__device__ __forceinline__ RowAt row_at(int kind, int e0, int S, int sl, int g)
{
    if (kind == 0) return {e0 + g, 0, (size_t)(e0 + g) * S};
    if (SLICED) return {e0 + g, sl, (size_t)(e0 + g) * S + sl};
    const size_t es = (size_t)e0 * S + g;
    const int e = (int)(es / (size_t)S);
    return {e, (int)(es - (size_t)e * S), es};
}

// Observation rows of `net`'s input -> LDS (zeros beyond the input and beyond the launch's rows).  REC: the rows are written to the
// record's slot on the way (the observation the TTI's action is computed from -- unrounded, also for a bf16 net (BF)).  `sl`: a sliced
// launch's slice (see row_at).
template <bool REC, bool SLICED = false, bool BF = false>
__device__ __forceinline__ void net_load_rows(const PolicyNet &net, const PolicyIO &io, const PolicyRec &rec, int kind, int e0, int row0, int n_rows,
                                              float *cur, int tid, int sl = 0)
{
    load_rows<BF>(net.kp[0], 0, 0, cur, tid, [&](int r, int k) {
        const int g = row0 + r;
        if (kind == 0) return dense_at(io.obs_inter, REC ? rec.obs_inter : nullptr, e0 + g, e0 + n_rows, 10 * io.S, net.in_dim, k);
        if (g >= n_rows || k >= net.in_dim) return 0.0f;
        const size_t es = row_at<SLICED>(1, e0, io.S, sl, g).es;
        const int ko = net.layout == RANENV_NET_IN_MASK_OBS ? k - io.Us : k;
        if (ko < 0) return (float)io.mask_intra[es * io.Us + k];
        const float v = io.obs_intra[es * io.W + ko];
        if (REC && rec.obs_intra) rec.obs_intra[es * io.W + ko] = v;
        return v;
    });
}

// A wave's 32 x 32 output tile `nt` of a bf16 layer: per 32 k one 16-byte load of W per block column (row c of the block, k = 8 q ..
// + 7: contiguous in the packed copy), one 16-byte LDS read of X per block row, 4 MFMAs; the next W loads are requested ahead
__device__ __forceinline__ void tile_bf16(f32x4 (&acc)[2][2], const __bf16 *W, const __bf16 *x, int K, int ldi, int nt, int q, int c)
{
    const bf16x8 *w0 = (const bf16x8 *)(W + (size_t)(nt * 32 + c) * K) + q;
    const bf16x8 *w1 = (const bf16x8 *)(W + (size_t)(nt * 32 + 16 + c) * K) + q;
    const __bf16 *x0 = x + c * ldi + 8 * q, *x1 = x + (16 + c) * ldi + 8 * q;
    bf16x8 b0 = w0[0], b1 = w1[0];
    for (int k0 = 0; k0 < K; k0 += 32) {
        const int kn = (k0 + 32 < K ? k0 + 32 : k0) >> 3;
        const bf16x8 nb0 = w0[kn], nb1 = w1[kn];
        const bf16x8 a0 = *(const bf16x8 *)(x0 + k0), a1 = *(const bf16x8 *)(x1 + k0);
        acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, b1, acc[1][1], 0, 0, 0);
        b0 = nb0; b1 = nb1;
    }
}

// The layers of `net`, its packed copy at `wb`, on the 32 rows in `cur`; on return `cur` holds the output layer's rows (f32, stride
// net_ld(np[last])).  BF: a bf16 net -- bf16 rows in `cur` (stride net_ld16) and between the layers, bf16 W.
// KEEP (the PPO update's backward pass reads them): every layer's rows stay -- layer l writes behind its input rows, at cur + 32 net_ld(kp[l])
// floats (BF: 32 net_ld16(kp[l]) bf16, half as many floats), so `nxt` is cur + 32 net_ld(kp[0]) (BF: cur + 16 net_ld16(kp[0])) on entry;
// on return `cur` holds the output layer's rows and `nxt` points behind them.
template <bool BF = false, bool KEEP = false>
__device__ __forceinline__ void net_layers(const PolicyNet &net, const float *wb, float *&cur, float *&nxt, int lane, int wave)
{
    const int q = lane >> 4, c = lane & 15;
    for (int l = 0; l < net.n_layers; l++) {
        const bool last = l == net.n_layers - 1;
        const int K = net.kp[l], N = net.np[l], ldi = BF ? net_ld16(K) : net_ld(K), ldo = BF && !last ? net_ld16(N) : net_ld(N);
        const float *W = wb + net.w_off[l], *bias = wb + net.b_off[l];
        for (int nt = wave; nt < N / 32; nt += 4) {
            f32x4 acc[2][2];
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int j = 0; j < 2; j++) acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            if constexpr (BF) tile_bf16(acc, (const __bf16 *)W, (const __bf16 *)cur, K, ldi, nt, q, c);
            else {
            const float4 *w0 = (const float4 *)(W + (size_t)(nt * 32 + c) * K) + q;
            const float4 *w1 = (const float4 *)(W + (size_t)(nt * 32 + 16 + c) * K) + q;
            const float *x0 = cur + c * ldi + 4 * q, *x1 = cur + (16 + c) * ldi + 4 * q;
            float4 b0 = w0[0], b1 = w1[0];
            for (int k0 = 0; k0 < K; k0 += 16) {
                const int kn = (k0 + 16 < K ? k0 + 16 : k0) >> 2;
                const float4 nb0 = w0[kn], nb1 = w1[kn];
                const float4 a0 = *(const float4 *)(x0 + k0), a1 = *(const float4 *)(x1 + k0);
                const float av[2][4] = {{a0.x, a0.y, a0.z, a0.w}, {a1.x, a1.y, a1.z, a1.w}};
                const float bv[2][4] = {{b0.x, b0.y, b0.z, b0.w}, {b1.x, b1.y, b1.z, b1.w}};
#pragma unroll
                for (int j = 0; j < 4; j++)
#pragma unroll
                    for (int mi = 0; mi < 2; mi++)
#pragma unroll
                        for (int ni = 0; ni < 2; ni++)
                            acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mi][j], bv[ni][j], acc[mi][ni], 0, 0, 0);
                b0 = nb0; b1 = nb1;
            }
            }
            // C/D map of the 16x16 block: column = lane & 15, row = 4 (lane >> 4) + register
#pragma unroll
            for (int mi = 0; mi < 2; mi++)
#pragma unroll
                for (int ni = 0; ni < 2; ni++) {
                    const int col = nt * 32 + ni * 16 + c;
                    const float bb = bias[col];
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        float v = acc[mi][ni][r] + bb;
                        if (!last) v = net.act == RANENV_ACT_RELU ? fmaxf(v, 0.0f) : tanhf(v);
                        if (BF && !last) ((__bf16 *)nxt)[(mi * 16 + q * 4 + r) * ldo + col] = (__bf16)v;
                        else nxt[(mi * 16 + q * 4 + r) * ldo + col] = v;
                    }
                }
        }
        __syncthreads();
        if constexpr (KEEP) { cur = nxt; nxt += NET_ROWS * (BF && !last ? ldo / 2 : ldo); }      // (bf16 rows: two elements per float)
        else { float *t = cur; cur = nxt; nxt = t; }
    }
}
__device__ __forceinline__ void net_layers(const PolicyNet &net, float *&cur, float *&nxt, int lane, int wave) { net_layers(net, net.w, cur, nxt, lane, wave); }

// ONE f32 layer `l` of `net` from the 32 rows at `in` (stride net_ld(kp[l])) to `out` (stride net_ld(np[l])): net_layers<false>'s tiling,
// k order, bias and activation, operation for operation -- the wide PPO update's forward pass (ranenv_ppo.hip), which decides per
// layer where the rows lie.  Ends without a barrier.  CHANGE THE TWO TOGETHER: the wide update is bit-equal to the plain one only
// while they agree, and tests/test_gpu_ppo_wide.py holds that.
__device__ __forceinline__ void net_layer_f32(const PolicyNet &net, int l, const float *wb, const float *in, float *out, int lane, int wave)
{
    const int q = lane >> 4, c = lane & 15;
    const bool last = l == net.n_layers - 1;
    const int K = net.kp[l], N = net.np[l], ldi = net_ld(K), ldo = net_ld(N);
    const float *W = wb + net.w_off[l], *bias = wb + net.b_off[l];
    for (int nt = wave; nt < N / 32; nt += 4) {
        f32x4 acc[2][2];
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
            for (int j = 0; j < 2; j++) acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        const float4 *w0 = (const float4 *)(W + (size_t)(nt * 32 + c) * K) + q;
        const float4 *w1 = (const float4 *)(W + (size_t)(nt * 32 + 16 + c) * K) + q;
        const float *x0 = in + c * ldi + 4 * q, *x1 = in + (16 + c) * ldi + 4 * q;
        float4 b0 = w0[0], b1 = w1[0];
        for (int k0 = 0; k0 < K; k0 += 16) {
            const int kn = (k0 + 16 < K ? k0 + 16 : k0) >> 2;
            const float4 nb0 = w0[kn], nb1 = w1[kn];
            const float4 a0 = *(const float4 *)(x0 + k0), a1 = *(const float4 *)(x1 + k0);
            const float av[2][4] = {{a0.x, a0.y, a0.z, a0.w}, {a1.x, a1.y, a1.z, a1.w}};
            const float bv[2][4] = {{b0.x, b0.y, b0.z, b0.w}, {b1.x, b1.y, b1.z, b1.w}};
#pragma unroll
            for (int j = 0; j < 4; j++)
#pragma unroll
                for (int mi = 0; mi < 2; mi++)
#pragma unroll
                    for (int ni = 0; ni < 2; ni++)
                        acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[mi][j], bv[ni][j], acc[mi][ni], 0, 0, 0);
            b0 = nb0; b1 = nb1;
        }
#pragma unroll
        for (int mi = 0; mi < 2; mi++)
#pragma unroll
            for (int ni = 0; ni < 2; ni++) {
                const int col = nt * 32 + ni * 16 + c;
                const float bb = bias[col];
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    float v = acc[mi][ni][r] + bb;
                    if (!last) v = net.act == RANENV_ACT_RELU ? fmaxf(v, 0.0f) : tanhf(v);
                    out[(mi * 16 + q * 4 + r) * ldo + col] = v;
                }
            }
    }
}

// The standard normal draw from words 0 and 1 of a Philox block (Box-Muller)
__device__ __forceinline__ double box_muller(const unsigned (&o)[4])
{
    const double u1 = ((double)o[0] + 1.0) * 0x1p-32, u2 = (double)o[1] * 0x1p-32;
    return sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
}

// The Gaussian sample, and SB3's clamp of a squashed Gaussian's log_std in front of it (HEAD / GAUSS_TANH, the SAC target and the SAC
// update: a = tanh(sample))
__device__ __forceinline__ double gauss_sample(double mu, double ls, double z) { return mu + exp(ls) * z; }
__device__ __forceinline__ double clamp_log_std(double ls) { return ls < -20.0 ? -20.0 : (ls > 2.0 ? 2.0 : ls); }

constexpr double HALF_LN_2PI = 0.9189385332046727;      // 0.5 ln(2 pi)
constexpr double LN_1E9 = 20.72326583694641;            // ln(1e9): -ln of the masked positions' std

// THE LOG-PROBABILITIES (include/ranenv.h, ranenv_trajectory "Arithmetic"), float64 from the float32 net outputs -- as macros: the
// acting kernels' epilogue and the PPO update expand the same expression text, and the epilogue's instructions stay what they were.
// Inter: an active position's term from its standardised action z and log_std, and what the j0 masked positions add
#define RANENV_INTER_LOGP_TERM(z, log_std) (((-0.5 * (z)) * (z) - (log_std)) - HALF_LN_2PI)
#define RANENV_INTER_LOGP_MASKED(j0) ((double)(j0) * (LN_1E9 - HALF_LN_2PI))
// Intra: the Categorical over the three float32 logits at choice ch (a statement: `out` = the log-probability).  The acting epilogue
// is its one user: the PPO update needs p and ln p of ALL three logits, so ranenv_ppo.hip's ppo_actor_row writes the same expressions
// out in the same order ((e0 + e1) + e2; (l - mx) - log(sum)).  CHANGE THE TWO TOGETHER: the update's re-evaluated logp is bit-equal
// to the recorded one only while they agree, and the GPU tests of the old log-probabilities hold that.
#define RANENV_INTRA_LOGP(out, l0, l1, l2, ch)                                                                      \
    {                                                                                                               \
        const double mx = fmax(fmax((double)l0, (double)l1), (double)l2);                                           \
        const double sum = (exp((double)l0 - mx) + exp((double)l1 - mx)) + exp((double)l2 - mx);                    \
        const double lc = (double)(ch == 0 ? l0 : (ch == 1 ? l1 : l2));                                             \
        out = (float)((lc - mx) - log(sum));                                                                        \
    }

// Enqueue a training kernel (ranenv_ppo.hip, ranenv_sac.hip) with `lds` bytes of dynamic LDS: the kernel's limit is raised to
// PPO_LDS_MAX once per kernel and process (the static of the kernel's own instance), the launch's error returned
template <auto KERNEL, class... A>
hipError_t launch_lds(dim3 grid, dim3 block, size_t lds, hipStream_t s, const A &...args)
{
    static const hipError_t attr = hipFuncSetAttribute((const void *)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PPO_LDS_MAX);
    if (attr != hipSuccess) return attr;
    hipLaunchKernelGGL(KERNEL, grid, block, lds, s, args...);
    return hipGetLastError();
}

}  // namespace
