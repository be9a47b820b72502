// ranenv_ppo_spread.hip -- the PPO update of ONE agent spread over the chip (ranenv_ppo_bind_spread; include/ranenv.h "One agent over
// the chip").  ranenv_ppo.hip gives a policy pair to one workgroup, which walks every row and passes over every parameter alone; here an
// optimiser step is three launches on the caller's stream, blockIdx.y the kind (0 inter, 1 intra: two independent optimisers, each with
// its own step count -- a kind whose steps are used up returns at once):
//   pass     min(tiles of the minibatch, slabs) workgroups per kind.  Workgroup w walks tiles w, w + grid, ... in ascending order and does
//            per tile what ranenv_ppo_body.hpp does between its barriers -- the same ranenv_ppo_parts.hpp functions on the same LDS plan,
//            plain or wide -- with the backward pass adding into gradient slab w, and writes its rows' statistics to wstat[w].  Every
//            workgroup computes the minibatch's advantage mean and std itself: the same function in the same order, the same bits.
//   reduce   elementwise over the kind's packed floats (actor, then critic), PPO_SPREAD_BLOCK per block: g[i] = the used slabs' [i]
//            summed in ascending slab order, the cells zeroed for the next step; a float64 sum of squares per block (ppo_sum's slot order).
//   apply    elementwise: every block adds up ALL block partials in ascending order -- the joint norm --, takes ppo_clip_scale and
//            adam_step at counter t0 + step + 1 and runs adam_elem on its elements, in place in the buffers the acting kernels read.
//            Block 0 keeps the epoch's statistics and, at the kind's last step, stores the counter; dev_grad is the last step's g.
// Whatever a launch writes -- weights, slabs, g, partials, running sums, the counter -- is read by LATER launches only (ranenv_sac.hip's
// rule): no cooperative launch, no grid-wide barrier, no flag, no atomics.  The step counter is read as t0 for the whole call: the first
// pass copies it to a cell of the binding's (t0), every apply reads that cell, and the last apply's block 0 stores t0 + steps to the
// counter, which no block of an apply reads.  The result is a function of the inputs and of min(tiles, slabs) alone; with one slab the
// tile order and the adds are the plain kernel's.
#include "ranenv_ppo_parts.hpp"

namespace {

__device__ __forceinline__ long long spread_floats(const PpoArgs &A, int kind) { return A.net[kind][0].floats + A.net[kind][1].floats; }

template <bool WIDE>
__device__ __forceinline__ void spread_pass(const PpoSpreadArgs &P)
{
    extern __shared__ float lds[];
    const PpoArgs &A = P.a;
    const ranenv_ppo_hparams &hp = P.hp;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, kind = (int)blockIdx.y;
    const PpoSpreadKind &K = P.k[kind];
    if (P.step >= K.steps) return;
    const PpoSpreadStep geo = ppo_spread_step(K.n, hp.minibatch, P.slabs, P.step);
    const int w = (int)blockIdx.x;
    if (w >= geo.grid) return;
    if (P.step == 0 && w == 0 && tid == 0) K.t0[0] = A.t[kind];
    const int n_nets = A.net[kind][1].net.n_layers > 0 ? 2 : 1;      // net 0 the actor, net 1 the critic

    double *red = (double *)lds, *rowstat = red + 256;
    int *rowidx = (int *)(rowstat + NET_ROWS * PPO_ROW_STATS);
    float *act = lds + PPO_FIXED / 4;
    const int S = A.S, c0 = geo.c0, nb = geo.nb;
    const long long n_record = (long long)A.T * A.B * (kind == 0 ? 1 : S);
    const int32_t *list = A.order[kind] + (size_t)geo.ep * (size_t)A.order_stride[kind];
    const double wrow = 1.0 / (double)nb;
    float *const slab = K.slab + (size_t)w * (size_t)K.slab_stride;
    float *const wpark = WIDE ? K.park + (size_t)w * (size_t)K.park_stride : nullptr;      // (the workgroup's parked rows)
    PpoEpoch st;                               // (thread 0's: this workgroup's tiles)

    double a_mean = 0.0, a_den = 1.0;
    if (hp.adv_norm)
        ppo_adv_norm(red, nb, tid, [&](int k) {
            const int i = list[c0 + k];
            return i < 0 || i >= n_record ? 0.0 : (double)A.traj.adv[ppo_cell(kind, i, S)];
        }, a_mean, a_den);

#pragma unroll 1
    for (int t0 = w * NET_ROWS; t0 < nb; t0 += geo.grid * NET_ROWS) {
        __syncthreads();                       // (the previous tile's backward pass and statistics are read)
        ppo_list_rows(rowidx, list, c0, t0, nb, n_record, tid);
#pragma unroll 1
        for (int k = 0; k < n_nets; k++) {
            const PpoNet &pn = A.net[kind][k];
            const PolicyNet &net = pn.net;
            const float *wt = pn.w;
            float *g = slab + (k == 0 ? 0 : A.net[kind][0].floats);
            __syncthreads();                   // (the tile's rows are listed; the actor's backward pass has read its rows)
            float *cur = act, *nxt = act + NET_ROWS * net_ld(net.kp[0]);
            ppo_load_rows(net, A, kind, rowidx, cur, tid);
            __syncthreads();
            if constexpr (WIDE) cur = ppo_forward_wide(net, wt, act, act + ppo_wide_floats(net), wpark, tid);
            else net_layers<false, true>(net, wt, cur, nxt, lane, wave);
            if (tid < NET_ROWS) {
                const int i = rowidx[tid], np = net.np[net.n_layers - 1];
                float *o = cur + tid * net_ld(np);
                double *rs = rowstat + tid * PPO_ROW_STATS;
                if (k == 0) ppo_actor_row(A, hp, kind, i, np, o, rs, wrow, a_mean, a_den);
                else rs[5] = ppo_critic_row(o, i, [&] { return A.traj.vtarg[ppo_cell(kind, i, S)]; }, hp.vf_coeff, wrow);
            }
            __syncthreads();
            if constexpr (WIDE) ppo_backward<true>(net, wt, g, cur, tid, act, act + ppo_wide_floats(net), wpark);
            else ppo_backward(net, wt, g, cur, tid);
        }
        if (tid == 0) ppo_tile_stats(st, rowstat, PPO_ROW_STATS, n_nets == 2);      // (the barriers above have published the rows')
    }
    if (tid == 0) {
        double *out = K.wstat + (size_t)w * PPO_SPREAD_STATS;
        out[0] = st.pl; out[1] = st.ent; out[2] = st.kl; out[3] = st.cf; out[4] = st.rows; out[5] = st.vl;
    }
}

__global__ void __launch_bounds__(256) ranenv_ppo_spread_pass_kernel(PpoSpreadArgs P) { spread_pass<false>(P); }
__global__ void __launch_bounds__(256) ranenv_ppo_spread_pass_kernel_wide(PpoSpreadArgs P) { spread_pass<true>(P); }

// Element e of the kind's packed floats: the actor's below its floats, the critic's behind
#define SPREAD_AT(field, e) ((e) < af ? A.net[kind][0].field + (e) : A.net[kind][1].field + ((e) - af))

__global__ void __launch_bounds__(256) ranenv_ppo_spread_reduce_kernel(PpoSpreadArgs P)
{
    __shared__ double red[256];
    const PpoArgs &A = P.a;
    const int tid = (int)threadIdx.x, kind = (int)blockIdx.y;
    const PpoSpreadKind &K = P.k[kind];
    if (P.step >= K.steps || (int)blockIdx.x >= K.blocks) return;
    const int used = ppo_spread_step(K.n, P.hp.minibatch, P.slabs, P.step).grid;
    const long long af = A.net[kind][0].floats, floats = spread_floats(A, kind);
    double s = 0.0;
#pragma unroll 1
    for (int j = 0; j < PPO_SPREAD_BLOCK / 256; j++) {
        const long long e = (long long)blockIdx.x * PPO_SPREAD_BLOCK + j * 256 + tid;
        if (e >= floats) break;
        float *p = K.slab + e;
        float g = *p;
        *p = 0.0f;
#pragma unroll 1
        for (int u = 1; u < used; u++) {
            p += K.slab_stride;
            g = g + *p;
            *p = 0.0f;
        }
        *SPREAD_AT(g, e) = g;
        s += (double)g * (double)g;
    }
    const double tot = ppo_sum(red, s, tid);
    if (tid == 0) K.bpart[blockIdx.x] = tot;
}

__global__ void __launch_bounds__(256) ranenv_ppo_spread_apply_kernel(PpoSpreadArgs P)
{
    const PpoArgs &A = P.a;
    const ranenv_ppo_hparams &hp = P.hp;
    const int tid = (int)threadIdx.x, kind = (int)blockIdx.y;
    const PpoSpreadKind &K = P.k[kind];
    if (P.step >= K.steps || (int)blockIdx.x >= K.blocks) return;
    double tot = 0.0;
#pragma unroll 1
    for (int b = 0; b < K.blocks; b++) tot += K.bpart[b];
    const double norm = sqrt(tot);
    const float sc = (float)ppo_clip_scale(hp.grad_clip, norm);
    const int t_call = K.t0[0];
    const AdamStep adam = adam_step(hp.lr, hp.beta1, hp.beta2, hp.eps, t_call + P.step + 1);
    const bool last = P.step == K.steps - 1;
    const long long af = A.net[kind][0].floats, floats = spread_floats(A, kind);
    float *const grad = last && A.grad ? A.grad + (size_t)kind * (size_t)A.grad_stride : nullptr;
#pragma unroll 1
    for (int j = 0; j < PPO_SPREAD_BLOCK / 256; j++) {
        const long long e = (long long)blockIdx.x * PPO_SPREAD_BLOCK + j * 256 + tid;
        if (e >= floats) break;
        const float g = *SPREAD_AT(g, e);
        if (grad) grad[e] = g;
        adam_elem(*SPREAD_AT(w, e), *SPREAD_AT(m, e), *SPREAD_AT(v, e), g * sc, adam);
    }
    if (blockIdx.x != 0 || tid != 0) return;
    // ---- block 0: the epoch's statistics and the counter ---------------------------------------------------------------------------
    const PpoSpreadStep geo = ppo_spread_step(K.n, hp.minibatch, P.slabs, P.step);
    PpoEpoch st;
    if (geo.mb > 0) { st.pl = K.run[0]; st.vl = K.run[1]; st.ent = K.run[2]; st.kl = K.run[3]; st.cf = K.run[4]; st.gn = K.run[5]; st.rows = K.run[6]; st.n_mb = (int)K.run[7]; }
#pragma unroll 1
    for (int u = 0; u < geo.grid; u++) {
        const double *ws = K.wstat + (size_t)u * PPO_SPREAD_STATS;
        st.pl += ws[0]; st.ent += ws[1]; st.kl += ws[2]; st.cf += ws[3]; st.rows += ws[4]; st.vl += ws[5];
    }
    st.gn += norm * (double)geo.nb;
    st.n_mb += 1;
    if (geo.mb == ppo_spread_per_epoch(K.n, hp.minibatch) - 1) ppo_epoch_stats(A.stats + ((size_t)kind * (size_t)A.max_epochs + geo.ep) * RANENV_PPO_STATS, st, K.n);
    else { K.run[0] = st.pl; K.run[1] = st.vl; K.run[2] = st.ent; K.run[3] = st.kl; K.run[4] = st.cf; K.run[5] = st.gn; K.run[6] = st.rows; K.run[7] = (double)st.n_mb; }
    if (last) A.t[kind] = t_call + K.steps;
}
#undef SPREAD_AT

}  // namespace

namespace ranenv_dev {

hipError_t launch_ppo_spread_step(hipStream_t s, size_t lds, const PpoSpreadArgs &a, bool wide)
{
    int grid = 0, blocks = 0;
    for (int k = 0; k < 2; k++) {
        if (a.step >= a.k[k].steps) continue;
        const int g = ppo_spread_step(a.k[k].n, a.hp.minibatch, a.slabs, a.step).grid;
        grid = g > grid ? g : grid;
        blocks = a.k[k].blocks > blocks ? a.k[k].blocks : blocks;
    }
    if (grid == 0) return hipSuccess;
    const dim3 pass((unsigned)grid, 2), elem((unsigned)blocks, 2), block(256);
    const hipError_t e = wide ? launch_lds<ranenv_ppo_spread_pass_kernel_wide>(pass, block, lds, s, a) : launch_lds<ranenv_ppo_spread_pass_kernel>(pass, block, lds, s, a);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ranenv_ppo_spread_reduce_kernel, elem, block, 0, s, a);
    hipLaunchKernelGGL(ranenv_ppo_spread_apply_kernel, elem, block, 0, s, a);
    return hipGetLastError();
}

}  // namespace ranenv_dev
