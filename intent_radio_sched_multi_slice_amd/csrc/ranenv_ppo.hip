// ranenv_ppo.hip -- the PPO update of the bound IBSched nets on the device (ranenv_ppo_update, include/ranenv.h "PPO update"): one
// workgroup per (population member, agent kind) runs that member's whole SGD schedule -- epochs x minibatches of clipped-surrogate
// loss, backward pass, joint gradient clip and Adam -- in one launch.  Nothing is shared between workgroups: no atomics, no reduction
// across them, one summation order.
//
// Per 32-row tile of a minibatch the workgroup gathers the indexed record rows into LDS and runs the net forward with the acting
// launches' own layers (net_layers<false, true>, ranenv_net.hpp), every layer's rows staying in LDS: buffer 0 the input rows, buffer
// l + 1 layer l's output, back to back.  The loss gradient at the outputs (float64 per row, rounded once) overwrites the output rows,
// and the backward pass walks the layers down, on the f32 matrix cores (v_mfma_f32_16x16x4_f32):
//   dW[n][k] += sum_r dZ[r][n] A[r][k]     16 x 16 blocks of W, 8 MFMAs each (the 32 rows are the reduction), added to the workgroup's
//                                          gradient scratch in global memory by plain load-add-store -- a wave owns its blocks
//   db[n]    += sum_r dZ[r][n]             a thread per column, rows in ascending order
//   dZ'[r][k] = (sum_n dZ[r][n] W[n][k]) act'(A[r][k])     32 x 16 blocks, written IN PLACE over A (a barrier behind dW, which read it)
// so the LDS need is one net's rows of all layers, not twice that.  Rows beyond the minibatch and padded columns are exact zeros all the
// way: a dead row's dZ is 0, a padded column's W and b are 0 and stay 0 under Adam (g = 0, m = v = 0).
// The weights this launch reads were written by the launch itself one minibatch earlier: the scalar cache does not see those vector
// stores, hence the weight-read rule stated at ppo_tile (ranenv_ppo_parts.hpp), which Adam's own loads follow too.
// Non-shared intra policies (ranenv_ppo_bind_slices, ranenv_ppo_update_slices) train in a launch of 1 + S workgroups of the same body: one
// for the inter pair and one per slice, each on its own rows, nets, counter, statistics and gradient block.
// Nets beyond that LDS plan train under the WIDE plan (ranenv_ppo_bind_wide; "the wide plan" below): two row buffers in LDS, every
// layer's input rows parked in a scratch of the workgroup's own in global memory -- written and read back by vector loads and stores
// at lane-dependent addresses behind workgroup barriers, as the weights are -- and the same arithmetic in the same order.
// Every step the training kernels share -- the backward pass, the workgroup sum, Adam, and the steps of a minibatch around the tile loop
// (advantage mean and std, row list, clipped surrogate, critic row, joint norm and clip, statistics) -- is a function of
// ranenv_ppo_parts.hpp, stated once: the kernels here, the spread update (ranenv_ppo_spread.hip) and the SAC update (ranenv_sac.hip)
// call them; the fixed LDS region (PPO_FIXED, PPO_ROW_STATS) and the 32-row tile itself stand there too, once each: ppo_tile for the
// IBSched nets (this file's six kernels and the spread pass) and ppo_head_tile for the head pair (the head kernel and its spread pass).
#include "ranenv_ppo_parts.hpp"

namespace {

// The update of workgroup (member, kind) = (blockIdx.x, blockIdx.y).  MIXED (a mixed population, ranenv_ppo_bind_mixed): a one-net
// workgroup on the member's OWN shape -- net k's descriptor is entry `member` of the role's device table, parked in the fixed LDS region
// at entry (the launch never writes a descriptor; A.net[kind][k].net, member 0's, says only whether the role is bound), its packed floats
// entry `member` of the binding's per-member array.  The rows lie in LDS at the member's own strides; w, m, v and g at member x stride
// as ever.  The body is one function template that each of the six kernels calls; its steps are ranenv_ppo_parts.hpp's functions, the
// tile of a minibatch (ppo_tile) among them.
// WIDE (ranenv_ppo_bind_wide): the forward and backward pass of a tile follow the wide plan above, on the workgroup's share of Y.scratch;
// every other line of the body is the same.
// SLICES (ranenv_ppo_bind_slices: one intra actor / critic pair per slice): a launch of 1 + S workgroups -- workgroup 0 is (member 0,
// inter), workgroup 1 + s is (`mem` = s, intra): slice s's copy of the intra nets stands at s x the slot's slice stride as a member's
// does, its share of the row list is first[1][s] .. first[1][s + 1], and hp[0] serves all.  What differs is where a workgroup finds its
// work: `mem`, `kind` and `wg` -- the workgroup's number among the call's, where its step counter, statistics, gradient block and parked
// rows lie -- at the body's top.
static_assert(PPO_FIXED >= (256 + NET_ROWS * PPO_ROW_STATS) * 8 + NET_ROWS * 4 + 2 * (int)sizeof(PolicyNet), "the fixed LDS region holds the two parked descriptors");

template <bool MIXED, bool WIDE, bool SLICES>
__device__ __forceinline__ void ppo_update_body(const PpoArgs &A, const PpoMixed &X, const PpoWide &Y)
{
    extern __shared__ float lds[];
    const int tid = (int)threadIdx.x;
    const int mem = SLICES ? ((int)blockIdx.x > 0 ? (int)blockIdx.x - 1 : 0) : (int)blockIdx.x, kind = SLICES ? ((int)blockIdx.x > 0 ? 1 : 0) : (int)blockIdx.y;
    const int wg = SLICES ? (int)blockIdx.x : mem * 2 + kind;
    if (A.net[kind][0].net.n_layers == 0) return;
    const ranenv_ppo_hparams &hp = A.hp[SLICES ? 0 : mem];
    const int epochs = hp.epochs, minibatch = hp.minibatch;
    if (epochs <= 0 || minibatch < 1) return;          // (minibatch < 1: the host refuses it)
    const int lo = A.first[kind][mem], n = A.first[kind][mem + 1] - lo;
    if (n <= 0) return;
    const int n_nets = A.net[kind][1].net.n_layers > 0 ? 2 : 1;      // net 0 the actor, net 1 the critic

    double *red = (double *)lds, *rowstat = red + 256;
    int *rowidx = (int *)(rowstat + NET_ROWS * PPO_ROW_STATS);
    float *act = lds + PPO_FIXED / 4;
    const PolicyNet *park = (const PolicyNet *)(rowidx + NET_ROWS);
    long long fl0 = 0, fl1 = 0;
    if constexpr (MIXED) {
        constexpr int words = (int)(sizeof(PolicyNet) / sizeof(int));
        if (tid < 2 * words) {
            const int k = tid / words;
            ((int *)park)[tid] = ((const int *)(X.tab[kind][k] + mem))[tid - k * words];
        }
        fl0 = X.floats[kind * POP_MAX + mem];
        fl1 = X.floats[(2 + kind) * POP_MAX + mem];
        __syncthreads();
    }
    // Net k of this workgroup's member: its descriptor and its packed floats (a constexpr choice between LDS and the kernel argument)
    const auto net_at = [&](int k) -> const PolicyNet & { if constexpr (MIXED) return park[k]; else return A.net[kind][k].net; };
    const auto floats_of = [&](int k) -> long long { if constexpr (MIXED) return k == 0 ? fl0 : fl1; else return A.net[kind][k].floats; };
    const int S = A.S;
    const long long n_record = (long long)A.T * A.B * (kind == 0 ? 1 : S);
    int t = A.t[wg];
    float *const wpark = WIDE ? Y.scratch + (size_t)wg * (size_t)Y.stride : nullptr;      // (the workgroup's parked rows)

#pragma unroll 1
    for (int ep = 0; ep < epochs; ep++) {
        const int32_t *list = A.order[kind] + (size_t)ep * (size_t)A.order_stride[kind] + lo;
        PpoEpoch st;                           // (thread 0's)
#pragma unroll 1
        for (int c0 = 0; c0 < n; c0 += minibatch) {
            const int nb = n - c0 < minibatch ? n - c0 : minibatch;
            const double wrow = 1.0 / (double)nb;
#pragma unroll 1
            for (int k = 0; k < n_nets; k++) ppo_zero(A.net[kind][k].g + mem * A.net[kind][k].stride, floats_of(k), tid);
            double a_mean = 0.0, a_den = 1.0;
            if (hp.adv_norm)
                ppo_adv_norm(red, nb, tid, [&](int k) {
                    const int i = list[c0 + k];
                    return i < 0 || i >= n_record ? 0.0 : (double)A.traj.adv[ppo_cell(kind, i, S)];
                }, a_mean, a_den);

#pragma unroll 1
            for (int t0 = 0; t0 < nb; t0 += NET_ROWS)
                ppo_tile<WIDE>(A, hp, kind, n_nets, list, c0, t0, nb, n_record, wrow, a_mean, a_den, rowstat, rowidx, act, wpark, st, tid, net_at,
                               [&](int k) -> const float * { return A.net[kind][k].w + mem * A.net[kind][k].stride; },
                               [&](int k) { return A.net[kind][k].g + mem * A.net[kind][k].stride; });
            __syncthreads();

            // ---- joint norm, clip, Adam -------------------------------------------------------------------------------------------
            double s = 0.0;
#pragma unroll 1
            for (int k = 0; k < n_nets; k++) s = ppo_sq_sum(A.net[kind][k].g + mem * A.net[kind][k].stride, floats_of(k), tid, s);
            const double norm = sqrt(ppo_sum(red, s, tid));
            const float sc = (float)ppo_clip_scale(hp.grad_clip, norm);
            t += 1;
            const AdamStep adam = adam_step(hp.lr, hp.beta1, hp.beta2, hp.eps, t);
#pragma unroll 1
            for (int k = 0; k < n_nets; k++) {
                const PpoNet &pn = A.net[kind][k];
                const long long at = mem * pn.stride;
                ppo_adam(pn.w + at, pn.m + at, pn.v + at, pn.g + at, floats_of(k), sc, adam, tid);
            }
            st.gn += norm * (double)nb;
            st.n_mb += 1;
            __syncthreads();                   // (the next minibatch reads the new weights)
        }
        if (tid == 0) ppo_epoch_stats(A.stats + ((size_t)wg * (size_t)A.max_epochs + ep) * RANENV_PPO_STATS, st, n);
    }
    if (A.grad) {
        float *out = A.grad + (size_t)wg * (size_t)A.grad_stride;
#pragma unroll 1
        for (int k = 0; k < n_nets; k++) {
            ppo_grad_out(out, A.net[kind][k].g + mem * A.net[kind][k].stride, floats_of(k), tid);
            out += floats_of(k);
        }
    }
    if (tid == 0) A.t[wg] = t;
}

__global__ void __launch_bounds__(256) ranenv_ppo_update_kernel(PpoArgs A) { ppo_update_body<false, false, false>(A, PpoMixed{}, PpoWide{}); }
__global__ void __launch_bounds__(256) ranenv_ppo_update_kernel_mixed(PpoArgs A, PpoMixed X) { ppo_update_body<true, false, false>(A, X, PpoWide{}); }
__global__ void __launch_bounds__(256) ranenv_ppo_update_kernel_wide(PpoArgs A, PpoWide Y) { ppo_update_body<false, true, false>(A, PpoMixed{}, Y); }
__global__ void __launch_bounds__(256) ranenv_ppo_update_kernel_mixed_wide(PpoArgs A, PpoMixed X, PpoWide Y) { ppo_update_body<true, true, false>(A, X, Y); }
__global__ void __launch_bounds__(256) ranenv_ppo_update_kernel_slices(PpoArgs A) { ppo_update_body<false, false, true>(A, PpoMixed{}, PpoWide{}); }
__global__ void __launch_bounds__(256) ranenv_ppo_update_kernel_slices_wide(PpoArgs A, PpoWide Y) { ppo_update_body<false, true, true>(A, PpoMixed{}, Y); }

// ---- the head policies (ranenv_ppo_update_head; include/ranenv.h "PPO update of the head policies") ----------------------------------
// ONE workgroup trains the head actor, the head critic and the state-independent log_std [S] of SB3's Gaussian on a ranenv_collect_head
// record.  A body of its own beside ppo_update_body -- no population, no kinds, no mask, a third parameter tensor -- whose every
// step that the body has too is the same ranenv_ppo_parts.hpp function (ppo_zero, ppo_adv_norm, ppo_sq_sum, ppo_clip_scale, adam_step /
// ppo_adam, ppo_epoch_stats, ppo_grad_out) and whose tile is ppo_head_tile, the spread head update's too (ranenv_ppo_spread.hip).  Its
// own: log_std, sig[] and g_ls.
// log_std is a weight this launch rewrites: its working copy lies in the fixed LDS region (`lsw`, loaded and reloaded by lane j at a
// lane-dependent address behind Adam's own store of the same lane), never read through a wave-uniform address.  sig[j] = exp(log_std_j)
// in float64 is parked in the reduction slots between two ppo_sum calls (refilled per minibatch behind the advantage pass).
__global__ void __launch_bounds__(256) ranenv_ppo_update_kernel_head(PpoHeadArgs A)
{
    extern __shared__ float lds[];
    const int tid = (int)threadIdx.x;
    const ranenv_ppo_hparams &hp = A.hp;
    const int epochs = hp.epochs, minibatch = hp.minibatch, n = A.n_rows, S = A.S;
    if (epochs <= 0 || minibatch < 1 || n <= 0) return;      // (the host refuses or serves them without a launch)

    double *red = (double *)lds, *rowstat = red + 256, *sig = red;
    int *rowidx = (int *)(rowstat + NET_ROWS * PPO_HEAD_ROW_STATS);
    float *lsw = (float *)(rowidx + NET_ROWS);
    float *act = lds + PPO_FIXED / 4;
    const long long n_record = (long long)A.T * A.B;
    int t = A.t[0];
    if (tid < S) lsw[tid] = A.log_std[tid];
    __syncthreads();

#pragma unroll 1
    for (int ep = 0; ep < epochs; ep++) {
        const int32_t *list = A.order + (size_t)ep * (size_t)n;
        PpoEpoch st;                           // (thread 0's)
#pragma unroll 1
        for (int c0 = 0; c0 < n; c0 += minibatch) {
            const int nb = n - c0 < minibatch ? n - c0 : minibatch;
            const double wrow = 1.0 / (double)nb;
#pragma unroll 1
            for (int k = 0; k < 2; k++) ppo_zero(A.net[k].g, A.net[k].floats, tid);
            double g_ls = 0.0;                 // (thread j < S: d/d log_std_j of the minibatch, rows in order)
            double a_mean = 0.0, a_den = 1.0;
            if (hp.adv_norm)
                ppo_adv_norm(red, nb, tid, [&](int k) {
                    const int i = list[c0 + k];
                    return i < 0 || i >= n_record ? 0.0 : (double)A.traj.adv[i];
                }, a_mean, a_den);
            if (tid < S) sig[tid] = exp((double)lsw[tid]);      // (published by the tile loop's first barrier; the slots are free until the norm)

#pragma unroll 1
            for (int t0 = 0; t0 < nb; t0 += NET_ROWS)
                ppo_head_tile(A, list, c0, t0, nb, n_record, wrow, a_mean, a_den, rowstat, rowidx, lsw, sig, act, g_ls, st, tid, [&](int k) { return A.net[k].g; });
            __syncthreads();

            // ---- joint norm over actor, critic and log_std; clip; Adam with the one counter -----------------------------------------
            if (tid < S) A.ls_g[tid] = (float)g_ls;          // (rounded once; read back by this thread alone)
            double s = 0.0;
#pragma unroll 1
            for (int k = 0; k < 2; k++) s = ppo_sq_sum(A.net[k].g, A.net[k].floats, tid, s);
            if (tid < S) { const double x = (double)A.ls_g[tid]; s += x * x; }
            const double norm = sqrt(ppo_sum(red, s, tid));
            const float sc = (float)ppo_clip_scale(hp.grad_clip, norm);
            t += 1;
            const AdamStep adam = adam_step(hp.lr, hp.beta1, hp.beta2, hp.eps, t);
#pragma unroll 1
            for (int k = 0; k < 2; k++) ppo_adam(A.net[k].w, A.net[k].m, A.net[k].v, A.net[k].g, A.net[k].floats, sc, adam, tid);
            ppo_adam(A.log_std, A.ls_m, A.ls_v, A.ls_g, S, sc, adam, tid);
            if (tid < S) lsw[tid] = A.log_std[tid];          // (lane j reloads what lane j stored: the handle's copy the next collect acts on)
            st.gn += norm * (double)nb;
            st.n_mb += 1;
            __syncthreads();                   // (the next minibatch reads the new weights and log_std)
        }
        if (tid == 0) ppo_epoch_stats(A.stats + (size_t)ep * RANENV_PPO_STATS, st, n);
    }
    if (A.grad) {
        float *out = A.grad;
#pragma unroll 1
        for (int k = 0; k < 2; k++) {
            ppo_grad_out(out, A.net[k].g, A.net[k].floats, tid);
            out += A.net[k].floats;
        }
        if (tid < S) out[tid] = A.ls_g[tid];
    }
    if (tid == 0) A.t[0] = t;
}

}  // namespace

namespace ranenv_dev {

size_t ppo_lds_bytes(const PolicyNet &actor, const PolicyNet *critic)
{
    int n = ppo_act_floats(actor);
    if (critic && critic->n_layers > 0) { const int v = ppo_act_floats(*critic); n = v > n ? v : n; }
    return (size_t)PPO_FIXED + sizeof(float) * (size_t)n;
}

size_t ppo_wide_lds_bytes(const PolicyNet &actor, const PolicyNet *critic)
{
    int n = ppo_wide_floats(actor);
    if (critic && critic->n_layers > 0) { const int v = ppo_wide_floats(*critic); n = v > n ? v : n; }
    return (size_t)PPO_FIXED + sizeof(float) * (size_t)n;
}

long long ppo_wide_scratch(const PolicyNet &actor, const PolicyNet *critic)
{
    long long n = ppo_wide_scratch_floats(actor);
    if (critic && critic->n_layers > 0) { const long long v = ppo_wide_scratch_floats(*critic); n = v > n ? v : n; }
    return n;
}

hipError_t launch_ppo_update(hipStream_t s, int n_members, size_t lds, const PpoArgs &a, const PpoMixed *mixed, const PpoWide *wide)
{
    const dim3 grid((unsigned)n_members, 2), block(256);
    if (mixed && wide) return launch_lds<ranenv_ppo_update_kernel_mixed_wide>(grid, block, lds, s, a, *mixed, *wide);
    if (wide) return launch_lds<ranenv_ppo_update_kernel_wide>(grid, block, lds, s, a, *wide);
    if (mixed) return launch_lds<ranenv_ppo_update_kernel_mixed>(grid, block, lds, s, a, *mixed);
    return launch_lds<ranenv_ppo_update_kernel>(grid, block, lds, s, a);
}

hipError_t launch_ppo_update_slices(hipStream_t s, int n_slices, size_t lds, const PpoArgs &a, const PpoWide *wide)
{
    const dim3 grid(1u + (unsigned)n_slices), block(256);
    if (wide) return launch_lds<ranenv_ppo_update_kernel_slices_wide>(grid, block, lds, s, a, *wide);
    return launch_lds<ranenv_ppo_update_kernel_slices>(grid, block, lds, s, a);
}

hipError_t launch_ppo_update_head(hipStream_t s, size_t lds, const PpoHeadArgs &a) { return launch_lds<ranenv_ppo_update_kernel_head>(dim3(1, 1), dim3(256), lds, s, a); }

}  // namespace ranenv_dev
