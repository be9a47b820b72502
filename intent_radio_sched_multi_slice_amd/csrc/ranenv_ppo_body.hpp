// ranenv_ppo_body.hpp -- the body of the PPO update kernels (ranenv_ppo.hip expands it once per kernel: no include guard).  In scope where
// it is expanded: the kernel's arguments `A` (PpoArgs), `X` (PpoMixed) and `Y` (PpoWide), `constexpr bool MIXED` and `WIDE`, and the macros
// PPO_NET(k) / PPO_FLOATS(k) -- net k's descriptor and packed floats of this workgroup's member.
    extern __shared__ float lds[];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int mem = (int)blockIdx.x, kind = (int)blockIdx.y;
    if (A.net[kind][0].net.n_layers == 0) return;
    const ranenv_ppo_hparams &hp = A.hp[mem];
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
    int t = A.t[mem * 2 + kind];
    float *const wpark = WIDE ? Y.scratch + ((size_t)mem * 2 + kind) * (size_t)Y.stride : nullptr;      // (the workgroup's parked rows)

#pragma unroll 1
    for (int ep = 0; ep < epochs; ep++) {
        const int32_t *list = A.order[kind] + (size_t)ep * (size_t)A.order_stride[kind] + lo;
        double st_pl = 0.0, st_vl = 0.0, st_ent = 0.0, st_kl = 0.0, st_cf = 0.0, st_gn = 0.0, st_rows = 0.0;      // (thread 0's)
        int n_mb = 0;
#pragma unroll 1
        for (int c0 = 0; c0 < n; c0 += minibatch) {
            const int nb = n - c0 < minibatch ? n - c0 : minibatch;
            const double wrow = 1.0 / (double)nb;
#pragma unroll 1
            for (int k = 0; k < n_nets; k++) {
                float *g = A.net[kind][k].g + mem * A.net[kind][k].stride;
                const long long f = PPO_FLOATS(k);
#pragma unroll 1
                for (long long i = tid; i < f; i += 256) g[i] = 0.0f;
            }
            double a_mean = 0.0, a_den = 1.0;
            if (hp.adv_norm) {                 // one float64 pass over the minibatch's advantages (entries outside the record: 0)
                auto adv_at = [&](int k) {
                    const int i = list[c0 + k];
                    if (i < 0 || i >= n_record) return 0.0;
                    return (double)A.traj.adv[kind == 0 ? (size_t)i * (S + 1) : (size_t)(i / S) * (S + 1) + 1 + (i % S)];
                };
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

#pragma unroll 1
            for (int t0 = 0; t0 < nb; t0 += NET_ROWS) {
                __syncthreads();               // (the previous tile's backward pass and statistics are read)
                if (tid < NET_ROWS) {
                    int i = -1;
                    if (t0 + tid < nb) { i = list[c0 + t0 + tid]; if (i < 0 || i >= n_record) i = -1; }
                    rowidx[tid] = i;
                }
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
                        else {                 // the critic: 2 vf_coeff (V - vtarg) / rows
                            double vl = 0.0;
                            if (i < 0) o[0] = 0.0f;
                            else {
                                const double d = (double)o[0] - (double)A.traj.vtarg[kind == 0 ? (size_t)i * (S + 1) : (size_t)(i / S) * (S + 1) + 1 + (i % S)];
                                vl = d * d;
                                o[0] = (float)(((2.0 * d) * hp.vf_coeff) * wrow);
                            }
                            rs[5] = vl;
                        }
                    }
                    __syncthreads();
                    if constexpr (WIDE) ppo_backward<true>(net, w, g, cur, tid, act, act + ppo_wide_floats(net), wpark);
                    else ppo_backward(net, w, g, cur, tid);
                }
                if (tid == 0) {                // (rows 0..31 in order; the barriers above have published them)
#pragma unroll 1
                    for (int r = 0; r < NET_ROWS; r++) {
                        const double *rs = rowstat + r * PPO_ROW_STATS;
                        st_pl += rs[0]; st_ent += rs[1]; st_kl += rs[2]; st_cf += rs[3]; st_rows += rs[4];
                        if (n_nets == 2) st_vl += rs[5];
                    }
                }
            }
            __syncthreads();

            // ---- joint norm, clip, Adam -------------------------------------------------------------------------------------------
            double s = 0.0;
#pragma unroll 1
            for (int k = 0; k < n_nets; k++) {
                const float *g = A.net[kind][k].g + mem * A.net[kind][k].stride;
                const long long f = PPO_FLOATS(k);
#pragma unroll 1
                for (long long i = tid; i < f; i += 256) { const double x = (double)g[i]; s += x * x; }
            }
            const double norm = sqrt(ppo_sum(red, s, tid));
            double sc = 1.0;
            if (hp.grad_clip > 0.0) { sc = hp.grad_clip / (norm + 1e-6); sc = sc < 1.0 ? sc : 1.0; }
            t += 1;
            const float step = (float)(hp.lr / (1.0 - ppo_powi(hp.beta1, t))), sbc2 = (float)sqrt(1.0 - ppo_powi(hp.beta2, t));
            const float b1 = (float)hp.beta1, omb1 = (float)(1.0 - hp.beta1), b2 = (float)hp.beta2, omb2 = (float)(1.0 - hp.beta2), eps = (float)hp.eps;
#pragma unroll 1
            for (int k = 0; k < n_nets; k++) {
                const PpoNet &pn = A.net[kind][k];
                const long long at = mem * pn.stride;
                ppo_adam(pn.w + at, pn.m + at, pn.v + at, pn.g + at, PPO_FLOATS(k), (float)sc, b1, omb1, b2, omb2, step, sbc2, eps, tid);
            }
            st_gn += norm * (double)nb;
            n_mb += 1;
            __syncthreads();                   // (the next minibatch reads the new weights)
        }
        if (tid == 0) {
            double *out = A.stats + (((size_t)mem * 2 + kind) * (size_t)A.max_epochs + ep) * RANENV_PPO_STATS;
            const double inv = 1.0 / (double)n;
            out[0] = st_pl * inv; out[1] = st_vl * inv; out[2] = st_ent * inv; out[3] = st_kl * inv; out[4] = st_cf * inv; out[5] = st_gn * inv;
            out[6] = st_rows; out[7] = (double)n_mb;
        }
    }
    if (A.grad) {
        float *out = A.grad + ((size_t)mem * 2 + kind) * (size_t)A.grad_stride;
#pragma unroll 1
        for (int k = 0; k < n_nets; k++) {
            const float *g = A.net[kind][k].g + mem * A.net[kind][k].stride;
            const long long f = PPO_FLOATS(k);
#pragma unroll 1
            for (long long i = tid; i < f; i += 256) out[i] = g[i];
            out += f;
        }
    }
    if (tid == 0) A.t[mem * 2 + kind] = t;
