// ranenv_ppo_body.hpp -- the body of the PPO update kernels (ranenv_ppo.hip expands it once per kernel: no include guard).  In scope where
// it is expanded: the kernel's arguments `A` (PpoArgs), `X` (PpoMixed) and `Y` (PpoWide), `constexpr bool MIXED`, `WIDE` and `SLICES`, and the
// macros PPO_NET(k) / PPO_FLOATS(k) -- net k's descriptor and packed floats of this workgroup's member -- and PPO_WG / PPO_WG_I, the
// workgroup's number among the call's (size_t / int): where its step counter, statistics, gradient block and parked rows lie.
// SLICES (ranenv_ppo_bind_slices): workgroup 0 is (member 0, inter), workgroup 1 + s is (`mem` = s, intra) -- slice s's copy of the intra
// nets stands at s x stride as a member's does, its share of the row list is first[1][s] .. first[1][s + 1], and hp[0] serves all.
    extern __shared__ float lds[];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int mem = SLICES ? ((int)blockIdx.x > 0 ? (int)blockIdx.x - 1 : 0) : (int)blockIdx.x, kind = SLICES ? ((int)blockIdx.x > 0 ? 1 : 0) : (int)blockIdx.y;
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
    const int S = A.S;
    const long long n_record = (long long)A.T * A.B * (kind == 0 ? 1 : S);
    int t = A.t[PPO_WG_I];
    float *const wpark = WIDE ? Y.scratch + PPO_WG * (size_t)Y.stride : nullptr;      // (the workgroup's parked rows)

#pragma unroll 1
    for (int ep = 0; ep < epochs; ep++) {
        const int32_t *list = A.order[kind] + (size_t)ep * (size_t)A.order_stride[kind] + lo;
        PpoEpoch st;                           // (thread 0's)
#pragma unroll 1
        for (int c0 = 0; c0 < n; c0 += minibatch) {
            const int nb = n - c0 < minibatch ? n - c0 : minibatch;
            const double wrow = 1.0 / (double)nb;
#pragma unroll 1
            for (int k = 0; k < n_nets; k++) ppo_zero(A.net[kind][k].g + mem * A.net[kind][k].stride, PPO_FLOATS(k), tid);
            double a_mean = 0.0, a_den = 1.0;
            if (hp.adv_norm)
                ppo_adv_norm(red, nb, tid, [&](int k) {
                    const int i = list[c0 + k];
                    return i < 0 || i >= n_record ? 0.0 : (double)A.traj.adv[ppo_cell(kind, i, S)];
                }, a_mean, a_den);

#pragma unroll 1
            for (int t0 = 0; t0 < nb; t0 += NET_ROWS) {
                __syncthreads();               // (the previous tile's backward pass and statistics are read)
                ppo_list_rows(rowidx, list, c0, t0, nb, n_record, tid);
                // ---- per net: forward, dL/d(output) per row, backward ---------------------------------------------------------------
#pragma unroll 1
                for (int k = 0; k < n_nets; k++) {
                    const PpoNet &pn = A.net[kind][k];
                    const PolicyNet &net = PPO_NET(k);
                    float *w = pn.w + mem * pn.stride, *g = pn.g + mem * pn.stride;
                    __syncthreads();           // (the tile's rows are listed; the actor's backward pass has read its rows)
                    float *cur = act, *nxt = act + NET_ROWS * net_ld(net.kp[0]);
                    ppo_load_rows(net, A, kind, rowidx, cur, tid);
                    __syncthreads();
                    if constexpr (WIDE) cur = ppo_forward_wide(net, w, act, act + ppo_wide_floats(net), wpark, tid);
                    else net_layers<false, true>(net, w, cur, nxt, lane, wave);
                    if (tid < NET_ROWS) {
                        const int i = rowidx[tid], np = net.np[net.n_layers - 1];
                        float *o = cur + tid * net_ld(np);
                        double *rs = rowstat + tid * PPO_ROW_STATS;
                        if (k == 0) ppo_actor_row(A, hp, kind, i, np, o, rs, wrow, a_mean, a_den);
                        else rs[5] = ppo_critic_row(o, i, [&] { return A.traj.vtarg[ppo_cell(kind, i, S)]; }, hp.vf_coeff, wrow);
                    }
                    __syncthreads();
                    if constexpr (WIDE) ppo_backward<true>(net, w, g, cur, tid, act, act + ppo_wide_floats(net), wpark);
                    else ppo_backward(net, w, g, cur, tid);
                }
                if (tid == 0) ppo_tile_stats(st, rowstat, PPO_ROW_STATS, n_nets == 2);      // (the barriers above have published the rows')
            }
            __syncthreads();

            // ---- joint norm, clip, Adam -------------------------------------------------------------------------------------------
            double s = 0.0;
#pragma unroll 1
            for (int k = 0; k < n_nets; k++) s = ppo_sq_sum(A.net[kind][k].g + mem * A.net[kind][k].stride, PPO_FLOATS(k), tid, s);
            const double norm = sqrt(ppo_sum(red, s, tid));
            const float sc = (float)ppo_clip_scale(hp.grad_clip, norm);
            t += 1;
            const AdamStep adam = adam_step(hp.lr, hp.beta1, hp.beta2, hp.eps, t);
#pragma unroll 1
            for (int k = 0; k < n_nets; k++) {
                const PpoNet &pn = A.net[kind][k];
                const long long at = mem * pn.stride;
                ppo_adam(pn.w + at, pn.m + at, pn.v + at, pn.g + at, PPO_FLOATS(k), sc, adam, tid);
            }
            st.gn += norm * (double)nb;
            st.n_mb += 1;
            __syncthreads();                   // (the next minibatch reads the new weights)
        }
        if (tid == 0) ppo_epoch_stats(A.stats + (PPO_WG * (size_t)A.max_epochs + ep) * RANENV_PPO_STATS, st, n);
    }
    if (A.grad) {
        float *out = A.grad + PPO_WG * (size_t)A.grad_stride;
#pragma unroll 1
        for (int k = 0; k < n_nets; k++) {
            ppo_grad_out(out, A.net[kind][k].g + mem * A.net[kind][k].stride, PPO_FLOATS(k), tid);
            out += PPO_FLOATS(k);
        }
    }
    if (tid == 0) A.t[PPO_WG_I] = t;
