// ranenv_policy.hip -- IBSched's trained policy networks on the device (RANENV_POLICY_NETWORK, include/ranenv.h): the inter-slice
// actor (masked diagonal Gaussian, agents/action_mask_model.py + agents/masked_action_distribution.py) and the intra-slice actors
// (Discrete(3), agents/ib_sched.py:394-470) as batched MLP forwards, one launch per net in front of a TTI.
//
// Every layer is a GEMM  Y[row][n] = act(sum_k X[row][k] W[n][k] + b[n])  with row = env (inter) or env x slice (intra), on the
// f32-input matrix cores (v_mfma_f32_16x16x4_f32: exact f32 products, f32 accumulation).  A workgroup owns NET_ROWS = 32 rows: their
// activations stay in LDS from the observation to the epilogue (two buffers of 32 x 516 floats at most), the weights are shared by
// all workgroups and come from L2.  Its four waves take the layer's 32-column tiles in turn; a wave's tile is 2 x 2 MFMA blocks of
// 16 x 16, four independent accumulators.  Per 16 k: one float4 of W per lane and block column (lane l: row c = l & 15 of the block,
// k = 4 (l >> 4) .. + 3), one float4 of X per block row from LDS, 16 MFMAs -- MFMA j of the step sums k = 4q + j, the same
// permutation on both operands.  The next W float4s are requested before the current step's MFMAs.
// A third agent kind, "head" (RANENV_POLICY_HEAD_NETWORK: the SB3 actors of SchedTWC / SchedColORAN on the head observation), shares
// everything but its distribution: a compile-time branch of the one body below.
//
// A net bound with RANENV_NET_BF16 (include/ranenv.h states the contract) takes the bf16 form of the same decomposition: its rows sit
// in LDS as bf16 (rounded to nearest even on the way in, and again behind every hidden layer's f32 bias + activation), its weights
// were rounded once at bind, and per 32 k a lane loads 16 bytes of W per block column (row c, k = 8 (l >> 4) .. + 7), reads 16 bytes
// of X per block row and issues 4 v_mfma_f32_16x16x32_bf16 -- 1/8 of the f32 form's MFMAs, half its weight bytes and LDS.  The
// output layer's rows are f32 in LDS: the epilogues do not know the difference.  Precision is per net and a compile-time parameter of
// the body (PREC: bit 0 the actor, bit 1 the critic of a recording launch -- a fused collect launch may pair a bf16 actor with an f32
// critic or the reverse): the kernels of f32 nets are the PREC = 0 instances and hold no bf16 code, launches with a bf16 net take the
// ranenv_*_bf16_* kernels.
#include "ranenv_net.hpp"

namespace {

constexpr unsigned POLICY_TAG = 0x504F4C00u;            // "POL\0" / "HEA\0": counter word c3 of the IBSched / head policies' Philox draws,
constexpr unsigned HEAD_TAG = 0x48454100u;              // + position (inter, head) or slice (intra)

// The Philox words of (env e, its episode and step, `tag`) under the launch's seed
__device__ __forceinline__ void draw_words(const PolicyIO &io, int e, unsigned tag, unsigned (&o)[4])
{
    philox4x32_10((unsigned)(io.env_id_base + e), (unsigned)io.episode_no[e], (unsigned)io.step_no[e], tag, (unsigned)io.seed,
                  (unsigned)(io.seed >> 32), o);
}

// ... and the standard normal draw from words 0 and 1 (box_muller, ranenv_net.hpp)
__device__ __forceinline__ double gauss_draw(const PolicyIO &io, int e, unsigned tag)
{
    unsigned o[4];
    draw_words(io, e, tag, o);
    return box_muller(o);
}

__device__ __forceinline__ int active_slices(const PolicyIO &io, int e)
{
    int n_act = 0;
    for (int s = 0; s < io.S; s++) n_act += io.mask_inter[(size_t)e * io.S + s] != 0 ? 1 : 0;
    return n_act;
}

// One workgroup's 32 rows of a launch through `net` and its epilogue.  kind 0: inter net, n_rows = envs; kind 1: intra net, n_rows =
// envs x S (row g of the launch = env e0 + g / S, slice g % S).  HEAD (compile time; kind 0): a head policy -- one row per env, the
// launch's io.obs_inter is the bound head observation [10*S], as the head kernel left it behind the previous TTI or reset; no masking
// (the step kernel applies the slice permutation and the inactive-slice rule to these scores as it does to a caller's), a clipped or
// tanh-squashed Gaussian (io.dist), and one column of logp / vf.
// REC (ranenv_collect / ranenv_collect_head): the same actor forward and epilogue -- the actions do not differ by a bit -- which also
// writes the TTI's record (observation and mask rows on their way into LDS; unclamped action, log-probability beside the handle's action
// buffers), then the critic `vnet` (n_layers 0 = none) on the same 32 rows, re-read from L2, through the same two LDS buffers.
// SLICED (compile time; kind 1, non-shared intra policies): a grid of S x tiles workgroups, tiles = ceil(n_rows / 32) with n_rows = envs.
// Workgroup sl * tiles + tile owns slice sl of envs e0 + 32 tile .. + 31 -- row g = 32 tile + r of the launch is (env e0 + g, slice sl) --
// and reads slice sl's copy of each net, net.w + sl * net.slice_stride (stride 0: one net for all slices).  Slice-major numbering: the
// workgroups resident at one time mostly walk one slice's weights (measured against tile * S + sl: never slower, 7 % faster with [512] x 3
// nets at B 16 384 S 5).
// PREC (compile time): bit 0 = `net` is a bf16 net, bit 1 = `vnet` is.
// POP (compile time; kinds 0 and 1, ranenv_set_population): n_rows = the launch's ENVS; member m of `pop` contributes the rows of its
// envs inside [e0, e0 + n_rows) -- pop_member_tiles, ranenv_internal.h -- in tiles of their own, workgroups numbered member-major (the
// co-resident ones walk one member's weights, as slice-major does for SLICED).  Every wave finds the workgroup's (member, tile) from
// blockIdx.x: lane m computes member m's tile count, an inclusive prefix sum over the wave and a ballot give the first member whose sum
// exceeds blockIdx.x; member and row range are broadcast and made scalar, so the weights at net.w + member * wa (vnet: wv; floats, 0 =
// one net for all members) are addressed as the one-net kernels address theirs.  From there on the workgroup is a one-net workgroup
// whose launch ends at the member's last row: row0 (the row map's g = row0 + r stays launch-relative) carries the member's row origin,
// n_rows becomes the member's end row, and the tail rows of the member's last tile are dead rows like the tail rows of a launch --
// zeros in LDS, nothing read from and nothing written to the next member's envs.
// POP = 2 (the mixed population kernels below, ranenv_set_population_policy_mixed / _value_mixed): `net_` / `vnet_` are entry 0 of the
// roles' device tables; the workgroup finds its member as under POP = 1 and takes ITS entries, whose .w point at the member's packed
// copies -- by reference: mem is scalar, the fields come by scalar loads as they are used -- and is from there on a one-net workgroup on
// that member's own shape and activation, the LDS buffers (ldm) sized from the member's own entries.
template <bool HEAD, bool REC, bool SLICED = false, int PREC = 0, int POP = 0>
__device__ __forceinline__ void policy_body(const PolicyNet &net_, const PolicyNet &vnet_, const PolicyIO &io, const PolicyRec &rec, int kind, int e0,
                                            int n_rows, float *lds, const PopMap *pop = nullptr, long long wa = 0, long long wv = 0)
{
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int S = io.S;
    const int tiles = SLICED ? (n_rows + NET_ROWS - 1) / NET_ROWS : 1, sl = SLICED ? (int)blockIdx.x / tiles : 0;
    int row0 = (SLICED ? (int)blockIdx.x - sl * tiles : (int)blockIdx.x) * NET_ROWS;
    int mem = 0;
    if constexpr (POP != 0) {
        PopShare sh{0, 0};
        const int mine = lane < pop->n ? pop_member_tiles(pop->first, lane, e0, n_rows, kind == 1 ? S : 1, sh) : 0;
        int upto = mine;
        for (int d = 1; d < WAVE; d <<= 1) {
            const int up = __shfl_up(upto, d);
            if (lane >= d) upto += up;
        }
        const unsigned long long owners = __ballot(upto > (int)blockIdx.x);
        if (owners == 0) return;                       // (a workgroup beyond the members' tiles: the host launches none)
        mem = __ffsll(owners) - 1;
        const int tile = (int)blockIdx.x - (__shfl(upto, mem) - __shfl(mine, mem));
        const int org = __shfl(sh.row0, mem);
        n_rows = __builtin_amdgcn_readfirstlane(org + __shfl(sh.rows, mem));
        row0 = __builtin_amdgcn_readfirstlane(org + tile * NET_ROWS);
        mem = __builtin_amdgcn_readfirstlane(mem);
    }
    const PolicyNet &net = POP == 2 ? (&net_)[mem] : net_, &vnet = POP == 2 ? (&vnet_)[mem] : vnet_;
    constexpr bool BFA = (PREC & 1) != 0, BFV = (PREC & 2) != 0;
    int ldm = net_ld_max<BFA>(net);
    if (REC && vnet.n_layers > 0) { const int lv = net_ld_max<BFV>(vnet); ldm = lv > ldm ? lv : ldm; }
    float *cur = lds, *nxt = lds + NET_ROWS * ldm;

    if (!REC || !rec.critic_only) {
    if (!HEAD && REC) {      // the masks of this TTI
        if (kind == 0 && rec.mask_inter)
            for (int i = tid; i < NET_ROWS * S; i += 256)
                if (row0 + i / S < n_rows) rec.mask_inter[(size_t)(e0 + row0) * S + i] = io.mask_inter[(size_t)(e0 + row0) * S + i];
        if (kind == 1 && rec.mask_intra)
            for (int i = tid; i < NET_ROWS * io.Us; i += 256)
                if (row0 + i / io.Us < n_rows) {
                    const size_t o = row_at<SLICED>(1, e0, S, sl, row0 + i / io.Us).es * io.Us + i % io.Us;
                    rec.mask_intra[o] = io.mask_intra[o];
                }
    }
    net_load_rows<REC, SLICED, BFA>(net, io, rec, kind, e0, row0, n_rows, cur, tid, sl);
    __syncthreads();
    net_layers<BFA>(net, SLICED ? net.w + sl * net.slice_stride : (POP == 1 ? net.w + mem * wa : net.w), cur, nxt, lane, wave);

    // ---- epilogue: actions ----------------------------------------------------------------------------------------------
    const int ld = net_ld(net.np[net.n_layers - 1]);
    if (kind == 0) {
        double *zrow = (double *)nxt;                  // REC: the draws z [32][S] for the rows' log-probabilities (the idle LDS buffer)
        for (int i = tid; i < NET_ROWS * S; i += 256) {
            const int r = i / S, j = i - r * S, g = row0 + r;
            if (g >= n_rows) continue;
            const int e = e0 + g;
            double score, raw, z = 0.0;
            if (HEAD) {
                const bool squash = io.dist == RANENV_HEAD_DIST_GAUSS_TANH;
                double a = (double)cur[r * ld + j];
                if (io.stochastic) {
                    const double ls = squash ? clamp_log_std((double)cur[r * ld + S + j]) : (double)io.log_std[j];
                    z = gauss_draw(io, e, HEAD_TAG + (unsigned)j);
                    a = gauss_sample(a, ls, z);
                }
                raw = a;
                score = squash ? tanh(a) : (a < -1.0 ? -1.0 : (a > 1.0 ? 1.0 : a));
            } else {
                const int n_act = active_slices(io, e);
                score = -1.0; raw = -1.0;              // masked position (sorted mask: the first S - n_act positions)
                if (j >= S - n_act) {
                    double m = (double)cur[r * ld + j];
                    if (io.stochastic) {
                        z = gauss_draw(io, e, POLICY_TAG + (unsigned)j);
                        m = gauss_sample(m, (double)cur[r * ld + S + j], z);
                    }
                    raw = m;
                    score = m < -1.0 ? -1.0 : (m > 1.0 ? 1.0 : m);
                }
            }
            io.scores[(size_t)e * S + j] = score;
            if (REC) {
                if (rec.action_inter) rec.action_inter[(size_t)e * S + j] = raw;
                zrow[i] = z;
            }
        }
        if (REC && rec.logp) {
            __syncthreads();
            for (int r = tid; r < NET_ROWS; r += 256) {
                const int g = row0 + r;
                if (g >= n_rows) continue;
                const int e = e0 + g;
                const int j0 = HEAD ? 0 : S - active_slices(io, e);      // the active positions: j0 .. S - 1
                double lp = 0.0;
                for (int j = j0; j < S; j++) {
                    const double z = zrow[r * S + j];
                    lp += RANENV_INTER_LOGP_TERM(z, (double)(HEAD ? io.log_std[j] : cur[r * ld + S + j]));
                }
                if (!HEAD) lp += RANENV_INTER_LOGP_MASKED(j0);
                float *out = rec.logp + (size_t)e * rec.cols;
                out[0] = (float)lp;
                if (!HEAD && !rec.intra_actor)
                    for (int s = 0; s < S; s++) out[1 + s] = 0.0f;
            }
        }
    } else {
        for (int r = tid; r < NET_ROWS; r += 256) {
            const int g = row0 + r;
            if (g >= n_rows) continue;
            const auto [e, s, es] = row_at<SLICED>(1, e0, S, sl, g);
            const float l0 = cur[r * ld], l1 = cur[r * ld + 1], l2 = cur[r * ld + 2];
            int ch = 0;
            if (!io.stochastic) {
                float best = l0;
                if (l1 > best) { ch = 1; best = l1; }
                if (l2 > best) ch = 2;
            } else {
                unsigned o[4];
                draw_words(io, e, POLICY_TAG + (unsigned)s, o);
                const double mx = fmax(fmax((double)l0, (double)l1), (double)l2);
                const double x0 = exp((double)l0 - mx), x1 = exp((double)l1 - mx), x2 = exp((double)l2 - mx);
                const double c0 = x0, c1 = x0 + x1, t = (double)o[2] * 0x1p-32 * (c1 + x2);
                ch = t < c0 ? 0 : (t < c1 ? 1 : 2);
            }
            io.intra[es] = (uint8_t)ch;
            if (REC) {
                if (rec.action_intra) rec.action_intra[es] = (uint8_t)ch;
                if (rec.logp) RANENV_INTRA_LOGP(rec.logp[(size_t)e * rec.cols + 1 + s], l0, l1, l2, ch)
            }
        }
    }
    }

    // ---- critic: the same rows through `vnet`, one value per row ------------------------------------------------------------
    if (REC && rec.vf && vnet.n_layers > 0) {
        __syncthreads();                               // (the epilogue read both buffers)
        cur = lds; nxt = lds + NET_ROWS * ldm;
        const PolicyRec none{};
        net_load_rows<false, SLICED, BFV>(vnet, io, none, kind, e0, row0, n_rows, cur, tid, sl);
        __syncthreads();
        net_layers<BFV>(vnet, SLICED ? vnet.w + sl * vnet.slice_stride : (POP == 1 ? vnet.w + mem * wv : vnet.w), cur, nxt, lane, wave);
        const int ldv = net_ld(vnet.np[vnet.n_layers - 1]);
        for (int r = tid; r < NET_ROWS; r += 256) {
            const int g = row0 + r;
            if (g >= n_rows) continue;
            if (kind == 0) {
                float *out = rec.vf + (size_t)(e0 + g) * rec.cols;
                out[0] = cur[r * ldv];
                if (!HEAD && !rec.intra_critic)
                    for (int s = 0; s < S; s++) out[1 + s] = 0.0f;
            } else {
                const RowAt at = row_at<SLICED>(1, e0, S, sl, g);
                rec.vf[(size_t)at.e * rec.cols + 1 + at.s] = cur[r * ldv];
            }
        }
    }
}

__global__ void __launch_bounds__(256) ranenv_policy_kernel(PolicyNet net, PolicyIO io, int kind, int e0, int n_rows)
{
    extern __shared__ float lds[];
    policy_body<false, false>(net, net, io, PolicyRec{}, kind, e0, n_rows, lds);
}

__global__ void __launch_bounds__(256) ranenv_policy_collect_kernel(PolicyNet net, PolicyNet vnet, PolicyIO io, PolicyRec rec, int kind, int e0, int n_rows)
{
    extern __shared__ float lds[];
    policy_body<false, true>(net, vnet, io, rec, kind, e0, n_rows, lds);
}

// Non-shared intra policies: the intra launch (kind 1) with one workgroup column per slice; n_envs rows per slice
__global__ void __launch_bounds__(256) ranenv_policy_sliced_kernel(PolicyNet net, PolicyIO io, int e0, int n_envs)
{
    extern __shared__ float lds[];
    policy_body<false, false, true>(net, net, io, PolicyRec{}, 1, e0, n_envs, lds);
}

__global__ void __launch_bounds__(256) ranenv_policy_sliced_collect_kernel(PolicyNet net, PolicyNet vnet, PolicyIO io, PolicyRec rec, int e0, int n_envs)
{
    extern __shared__ float lds[];
    policy_body<false, true, true>(net, vnet, io, rec, 1, e0, n_envs, lds);
}

__global__ void __launch_bounds__(256) ranenv_head_policy_kernel(PolicyNet net, PolicyIO io, int e0, int n_rows)
{
    extern __shared__ float lds[];
    policy_body<true, false>(net, net, io, PolicyRec{}, 0, e0, n_rows, lds);
}

__global__ void __launch_bounds__(256) ranenv_head_policy_collect_kernel(PolicyNet net, PolicyNet vnet, PolicyIO io, PolicyRec rec, int e0, int n_rows)
{
    extern __shared__ float lds[];
    policy_body<true, true>(net, vnet, io, rec, 0, e0, n_rows, lds);
}

// The same six with a bf16 net (PREC as in policy_body: 1 for the acting kernels, 1..3 for the recording ones)
template <int PREC>
__global__ void __launch_bounds__(256) ranenv_policy_bf16_kernel(PolicyNet net, PolicyIO io, int kind, int e0, int n_rows)
{
    extern __shared__ float lds[];
    policy_body<false, false, false, PREC>(net, net, io, PolicyRec{}, kind, e0, n_rows, lds);
}

template <int PREC>
__global__ void __launch_bounds__(256) ranenv_policy_bf16_collect_kernel(PolicyNet net, PolicyNet vnet, PolicyIO io, PolicyRec rec, int kind, int e0, int n_rows)
{
    extern __shared__ float lds[];
    policy_body<false, true, false, PREC>(net, vnet, io, rec, kind, e0, n_rows, lds);
}

template <int PREC>
__global__ void __launch_bounds__(256) ranenv_policy_bf16_sliced_kernel(PolicyNet net, PolicyIO io, int e0, int n_envs)
{
    extern __shared__ float lds[];
    policy_body<false, false, true, PREC>(net, net, io, PolicyRec{}, 1, e0, n_envs, lds);
}

template <int PREC>
__global__ void __launch_bounds__(256) ranenv_policy_bf16_sliced_collect_kernel(PolicyNet net, PolicyNet vnet, PolicyIO io, PolicyRec rec, int e0, int n_envs)
{
    extern __shared__ float lds[];
    policy_body<false, true, true, PREC>(net, vnet, io, rec, 1, e0, n_envs, lds);
}

template <int PREC>
__global__ void __launch_bounds__(256) ranenv_head_policy_bf16_kernel(PolicyNet net, PolicyIO io, int e0, int n_rows)
{
    extern __shared__ float lds[];
    policy_body<true, false, false, PREC>(net, net, io, PolicyRec{}, 0, e0, n_rows, lds);
}

template <int PREC>
__global__ void __launch_bounds__(256) ranenv_head_policy_bf16_collect_kernel(PolicyNet net, PolicyNet vnet, PolicyIO io, PolicyRec rec, int e0, int n_rows)
{
    extern __shared__ float lds[];
    policy_body<true, true, false, PREC>(net, vnet, io, rec, 0, e0, n_rows, lds);
}

// A population's launches (ranenv_set_population_policy / _value): kinds 0 and 1 of the IBSched nets, acting and recording, PREC as in
// policy_body (0: f32 nets).  n_envs: the launch's envs, whatever the kind; wa / wv: floats between two members' copies of net / vnet.
template <int PREC>
__global__ void __launch_bounds__(256) ranenv_policy_pop_kernel(PolicyNet net, PolicyIO io, PopMap pop, long long wa, int kind, int e0, int n_envs)
{
    extern __shared__ float lds[];
    policy_body<false, false, false, PREC, 1>(net, net, io, PolicyRec{}, kind, e0, n_envs, lds, &pop, wa, 0);
}

template <int PREC>
__global__ void __launch_bounds__(256) ranenv_policy_pop_collect_kernel(PolicyNet net, PolicyNet vnet, PolicyIO io, PolicyRec rec, PopMap pop, long long wa,
                                                                        long long wv, int kind, int e0, int n_envs)
{
    extern __shared__ float lds[];
    policy_body<false, true, false, PREC, 1>(net, vnet, io, rec, kind, e0, n_envs, lds, &pop, wa, wv);
}

// A mixed population's launches (ranenv_set_population_policy_mixed / _value_mixed): the same geometry, the member's descriptors from
// the roles' device tables (policy_body, POP = 2).
template <int PREC>
__global__ void __launch_bounds__(256) ranenv_policy_mixed_kernel(const PolicyNet *__restrict__ tab_a, PolicyIO io, PopMap pop, int kind, int e0, int n_envs)
{
    extern __shared__ float lds[];
    policy_body<false, false, false, PREC, 2>(*tab_a, *tab_a, io, PolicyRec{}, kind, e0, n_envs, lds, &pop);
}

template <int PREC>
__global__ void __launch_bounds__(256) ranenv_policy_mixed_collect_kernel(const PolicyNet *__restrict__ tab_a, const PolicyNet *__restrict__ tab_v, PolicyIO io,
                                                                          PolicyRec rec, PopMap pop, int kind, int e0, int n_envs)
{
    extern __shared__ float lds[];
    policy_body<false, true, false, PREC, 2>(*tab_a, *tab_v, io, rec, kind, e0, n_envs, lds, &pop);
}

// ---- SAC's soft Bellman target (ranenv_sac_targets; the arithmetic is spelled out in include/ranenv.h) -----------------------------
constexpr unsigned SAC_TAG = 0x53414300u;               // "SAC\0": counter word c3 of the target's Philox draws, + position

// The critics' input rows [next_obs | a32] of the workgroup's 32 rows -> `dst` (zeros beyond the input and beyond the call's rows):
// the observation re-read from L2, the actions from the registers of the threads that computed them (position tid + 256 k)
__device__ __forceinline__ void sac_critic_rows(const PolicyNet &q, const SacArgs &a, long long row0, const float (&a32)[2], float *dst, int tid)
{
    const int S = a.S, ld0 = net_ld(q.kp[0]);
    load_dense_rows(a.next_obs, row0, a.n, 10 * S, 10 * S, q.kp[0], 10 * S, 11 * S, dst, tid);
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const int i = tid + 256 * k;
        if (i < NET_ROWS * S) dst[(i / S) * ld0 + 10 * S + (i % S)] = a32[k];
    }
}

// A workgroup owns 32 rows: the actor on next_obs, the squashed-Gaussian epilogue (a', log pi), then the two critics on [next_obs | a']
// through the same two LDS buffers, then the target.  f32 nets only (the host refuses bf16 ones here).  S <= 16: a thread owns at most two (row, position) pairs.
__global__ void __launch_bounds__(256) ranenv_sac_target_kernel(PolicyNet actor, PolicyNet q1, PolicyNet q2, SacArgs a)
{
    extern __shared__ float lds[];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long row0 = (long long)blockIdx.x * NET_ROWS;
    const int S = a.S;
    int ldm = net_ld_max(actor);
    { const int lq = net_ld_max(q1); ldm = lq > ldm ? lq : ldm; }
    float *cur = lds, *nxt = lds + NET_ROWS * ldm;

    load_dense_rows(a.next_obs, row0, a.n, 10 * S, actor.in_dim, actor.kp[0], 0, 0, cur, tid);
    __syncthreads();
    net_layers(actor, cur, nxt, lane, wave);

    // ---- epilogue: a' = tanh(mu + exp(ls) z) and the positions' terms of log pi(a') (the idle LDS buffer) ------------------------
    const int ld = net_ld(actor.np[actor.n_layers - 1]);
    double *term = (double *)nxt;
    float a32[2] = {0.0f, 0.0f};
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const int i = tid + 256 * k;
        if (i >= NET_ROWS * S) continue;
        const int r = i / S, j = i - r * S;
        const long long g = row0 + r;
        if (g >= a.n) continue;
        const double ls = clamp_log_std((double)cur[r * ld + S + j]);
        double z = 0.0;
        if (a.stochastic) {
            unsigned o[4];
            philox4x32_10((unsigned)g, (unsigned)((unsigned long long)g >> 32), (unsigned)a.draw, SAC_TAG + (unsigned)j, (unsigned)a.seed,
                          (unsigned)(a.seed >> 32), o);
            z = box_muller(o);
        }
        const double aj = tanh(gauss_sample((double)cur[r * ld + j], ls, z));
        a32[k] = (float)aj;
        term[i] = ((((-0.5 * z) * z - ls) - HALF_LN_2PI)) - log((1.0 - aj * aj) + 1e-6);
        if (a.next_action) a.next_action[(size_t)g * S + j] = a32[k];
    }
    __syncthreads();
    const long long gr = row0 + tid;                   // threads 0..31: the row's log pi, Q values and target
    const bool own = tid < NET_ROWS && gr < a.n;
    double lp = 0.0;
    if (own) {
        for (int j = 0; j < S; j++) lp += term[tid * S + j];
        if (a.next_logp) a.next_logp[gr] = (float)lp;
    }

    // ---- the critics ---------------------------------------------------------------------------------------------------------------
    const int ldq = net_ld(q1.np[q1.n_layers - 1]);
    sac_critic_rows(q1, a, row0, a32, cur, tid);
    __syncthreads();                                   // (... and the terms are read: the critic's layers overwrite them)
    net_layers(q1, cur, nxt, lane, wave);
    const float v1 = own ? cur[tid * ldq] : 0.0f;
    sac_critic_rows(q2, a, row0, a32, nxt, tid);       // (into the idle buffer: threads 0..31 may still be reading Q1's rows)
    __syncthreads();
    { float *t = cur; cur = nxt; nxt = t; }
    net_layers(q2, cur, nxt, lane, wave);
    if (!own) return;
    const float v2 = cur[tid * ldq];
    if (a.q) { a.q[(size_t)gr * 2] = v1; a.q[(size_t)gr * 2 + 1] = v2; }
    const double nd = a.done[gr] ? 0.0 : 1.0;
    a.target[gr] = (float)((double)a.reward[gr] + nd * (a.gamma * (fmin((double)v1, (double)v2) - a.ent_coef * lp)));
}

// Enqueue KERNEL, its dynamic LDS limit raised to the widest net's need (2 x 32 x 516 floats = 129 KB) once per kernel
template <auto KERNEL, class... A>
hipError_t launch_kernel(dim3 grid, size_t lds, hipStream_t s, const A &...args)
{
    static const hipError_t attr = hipFuncSetAttribute((const void *)KERNEL, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                       (int)(sizeof(float) * 2 * NET_ROWS * net_ld(NET_MAX_WIDTH)));
    if (attr != hipSuccess) return attr;
    hipLaunchKernelGGL(KERNEL, grid, dim3(256), lds, s, args...);
    return hipSuccess;
}

using ranenv_dev::policy_lds_bytes;

// A kind's tables under a mixed population (PolicyNets::tab): actor, critic and the table of zeros, with the largest member's LDS need of each
struct MixedKind { const PolicyNet *tab_a, *tab_v, *tab_none; size_t lds_a, lds_v; };

// One agent kind's launch(es) of a TTI for envs [e0, e0 + n_envs): the actor `a` alone (rec null), or the recording launch -- actor +
// critic `vp` (null: none) fused, or, split, the actor's launch and then the critic alone (the kernel's critic_only mode).  THE GEOMETRY:
// kind 0 has one row per env; an intra launch (kind 1) has the flat env x S rows, or -- sliced, when its actor or its critic has a copy
// per slice -- one row per env in S x tiles workgroups (see policy_body).  pop non-null (a population's copies of the actor at stride
// wa, of the critic at wv; never with nets per slice): the sum of the members' tiles, by pop_member_tiles.  mx non-null (with pop): the
// mixed kernels on the kind's tables -- `a` / `vp` then only say which precision the role has and whether there is a critic, and the
// dynamic LDS is the largest member's need of the nets the launch runs, not member 0's.
hipError_t launch_kind(hipStream_t s, bool head, int kind, const PolicyNet &a, const PolicyNet *vp, const PolicyIO &io, const PolicyRec *rec,
                       int e0, int n_envs, bool split, const PopMap *pop = nullptr, long long wa = 0, long long wv = 0, const MixedKind *mx = nullptr)
{
    const bool sl = kind == 1 && (a.slice_stride != 0 || (vp && vp->slice_stride != 0));
    const int rows = kind == 1 && !sl ? n_envs * io.S : n_envs;
    unsigned tiles = (unsigned)((rows + NET_ROWS - 1) / NET_ROWS) * (sl ? (unsigned)io.S : 1u);
    if (pop) {
        if (head || sl) return hipErrorInvalidValue;
        tiles = 0;
        PopShare sh;
        for (int m = 0; m < pop->n; m++) tiles += (unsigned)pop_member_tiles(pop->first, m, e0, n_envs, kind == 1 ? io.S : 1, sh);
        if (tiles == 0) return hipSuccess;
    }
    const dim3 grid(tiles);
    const bool bfa = a.prec == RANENV_NET_BF16;
    if (!rec) {
        const size_t lds = mx ? mx->lds_a : policy_lds_bytes(a);
        if (mx) return bfa ? launch_kernel<ranenv_policy_mixed_kernel<1>>(grid, lds, s, mx->tab_a, io, *pop, kind, e0, n_envs)
                           : launch_kernel<ranenv_policy_mixed_kernel<0>>(grid, lds, s, mx->tab_a, io, *pop, kind, e0, n_envs);
        if (pop) return bfa ? launch_kernel<ranenv_policy_pop_kernel<1>>(grid, lds, s, a, io, *pop, wa, kind, e0, n_envs)
                            : launch_kernel<ranenv_policy_pop_kernel<0>>(grid, lds, s, a, io, *pop, wa, kind, e0, n_envs);
        if (sl) return bfa ? launch_kernel<ranenv_policy_bf16_sliced_kernel<1>>(grid, lds, s, a, io, e0, rows) : launch_kernel<ranenv_policy_sliced_kernel>(grid, lds, s, a, io, e0, rows);
        if (head) return bfa ? launch_kernel<ranenv_head_policy_bf16_kernel<1>>(grid, lds, s, a, io, e0, rows) : launch_kernel<ranenv_head_policy_kernel>(grid, lds, s, a, io, e0, rows);
        return bfa ? launch_kernel<ranenv_policy_bf16_kernel<1>>(grid, lds, s, a, io, kind, e0, rows) : launch_kernel<ranenv_policy_kernel>(grid, lds, s, a, io, kind, e0, rows);
    }
    const PolicyNet none{};               // (n_layers 0: no critic)
    auto launch = [&](const PolicyNet &v, const PolicyRec &rc) {
        const size_t x = mx ? mx->lds_a : policy_lds_bytes(a), y = v.n_layers > 0 ? (mx ? mx->lds_v : policy_lds_bytes(v)) : 0, lds = x > y ? x : y;
        auto as = [&](auto prec) {        // the recording kernels' PREC instance
            constexpr int P = decltype(prec)::value;
            if (sl) return launch_kernel<ranenv_policy_bf16_sliced_collect_kernel<P>>(grid, lds, s, a, v, io, rc, e0, rows);
            if (head) return launch_kernel<ranenv_head_policy_bf16_collect_kernel<P>>(grid, lds, s, a, v, io, rc, e0, rows);
            return launch_kernel<ranenv_policy_bf16_collect_kernel<P>>(grid, lds, s, a, v, io, rc, kind, e0, rows);
        };
        const int prec = (bfa ? 1 : 0) | (v.n_layers > 0 && v.prec == RANENV_NET_BF16 ? 2 : 0);
        if (pop) {
            auto pop_as = [&](auto p) {
                if (mx) return launch_kernel<ranenv_policy_mixed_collect_kernel<decltype(p)::value>>(grid, lds, s, mx->tab_a, v.n_layers > 0 ? mx->tab_v : mx->tab_none,
                                                                                                     io, rc, *pop, kind, e0, n_envs);
                return launch_kernel<ranenv_policy_pop_collect_kernel<decltype(p)::value>>(grid, lds, s, a, v, io, rc, *pop, wa, wv, kind, e0, n_envs);
            };
            switch (prec) {
            case 1: return pop_as(std::integral_constant<int, 1>{});
            case 2: return pop_as(std::integral_constant<int, 2>{});
            case 3: return pop_as(std::integral_constant<int, 3>{});
            }
            return pop_as(std::integral_constant<int, 0>{});
        }
        switch (prec) {
        case 1: return as(std::integral_constant<int, 1>{});
        case 2: return as(std::integral_constant<int, 2>{});
        case 3: return as(std::integral_constant<int, 3>{});
        }
        if (sl) return launch_kernel<ranenv_policy_sliced_collect_kernel>(grid, lds, s, a, v, io, rc, e0, rows);
        if (head) return launch_kernel<ranenv_head_policy_collect_kernel>(grid, lds, s, a, v, io, rc, e0, rows);
        return launch_kernel<ranenv_policy_collect_kernel>(grid, lds, s, a, v, io, rc, kind, e0, rows);
    };
    if (!split || rec->critic_only || !vp) return launch(vp ? *vp : none, *rec);
    if (const hipError_t e = launch(none, *rec); e != hipSuccess) return e;
    PolicyRec crit{};
    crit.vf = rec->vf; crit.cols = rec->cols; crit.intra_critic = rec->intra_critic; crit.critic_only = 1;
    return launch(*vp, crit);
}

}  // namespace

namespace ranenv_dev {

size_t policy_lds_bytes(const PolicyNet &net)
{
    return sizeof(float) * 2 * NET_ROWS * (size_t)(net.prec == RANENV_NET_BF16 ? net_ld_max<true>(net) : net_ld_max<false>(net));
}

hipError_t launch_policy(hipStream_t s, const PolicyNets &n, const PolicyIO &io, const PolicyRec *rec, int e0, int n_envs)
{
    const bool critics = rec && rec->critic_only;      // the critics' pass: a kind without a critic has no launch
    const PolicyNet *critic = rec ? n.critic : nullptr, *vintra = rec ? n.vintra : nullptr;
    const int split = rec ? rec->split : 0;
    hipError_t e = hipSuccess;
    // (a kind none of whose nets has a copy per member runs the one-net kernels, population or not)
    const bool pop0 = n.pop && (n.stride[0] != 0 || (critic && n.stride[2] != 0)), pop1 = n.pop && (n.stride[1] != 0 || (vintra && n.stride[3] != 0));
    // (a kind with a role of mixed member shapes: the mixed kernels on the roles' tables)
    const MixedKind mx0{n.tab[0], n.tab[2], n.tab_none, n.lds[0], n.lds[2]}, mx1{n.tab[1], n.tab[3], n.tab_none, n.lds[1], n.lds[3]};
    if (!critics || critic)
        e = launch_kind(s, n.head, 0, *n.actor, critic, io, rec, e0, n_envs, (split & 1) != 0, pop0 ? n.pop : nullptr, n.stride[0], n.stride[2],
                        pop0 && n.tab[0] ? &mx0 : nullptr);
    if (e == hipSuccess && n.intra && (!critics || vintra))
        e = launch_kind(s, false, 1, *n.intra, vintra, io, rec, e0, n_envs, (split & 2) != 0, pop1 ? n.pop : nullptr, n.stride[1], n.stride[3],
                        pop1 && n.tab[1] ? &mx1 : nullptr);
    return e != hipSuccess ? e : hipGetLastError();
}

hipError_t launch_sac_targets(hipStream_t s, const PolicyNet &actor, const PolicyNet &q1, const PolicyNet &q2, const SacArgs &a)
{
    const size_t x = policy_lds_bytes(actor), y = policy_lds_bytes(q1), lds = x > y ? x : y;
    const hipError_t e = launch_kernel<ranenv_sac_target_kernel>(dim3((unsigned)((a.n + NET_ROWS - 1) / NET_ROWS)), lds, s, actor, q1, q2, a);
    return e != hipSuccess ? e : hipGetLastError();
}

}  // namespace ranenv_dev
