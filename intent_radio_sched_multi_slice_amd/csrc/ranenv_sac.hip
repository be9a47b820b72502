// ranenv_sac.hip -- the SAC update on the device (ranenv_sac_update, include/ranenv.h "SAC update"): one gradient step of SB3's
// SAC.train is four launches on the caller's stream,
//   critic pass   the soft Bellman target of the minibatch's rows under the actor and the TARGET critics (ranenv_sac_target_kernel's
//                 rule, the coefficient read from device memory), both live critics' forward on [obs | action], dL/dQ = (Q - target) / n,
//                 the backward pass into the workgroup's gradient slab
//   apply         the critics' gradient = the used slabs summed in ascending order, Adam
//   actor pass    the actor's forward and squashed-Gaussian epilogue, both live critics -- AS UPDATED -- on [obs | a32], the smaller
//                 one's gradient at its input's action columns, the epilogue's gradient at the actor's outputs, the backward pass
//   apply         the actor's gradient and Adam, the entropy coefficient's step, polyak into the target critics, the statistics
// The rows of a minibatch are spread over workgroups: tiles of NET_ROWS rows, min(tiles, slabs) workgroups, workgroup w walks tiles
// w, w + grid, ... in ascending order and adds into gradient slab w by ppo_backward's plain load-add-store.  No atomics: the
// result is a function of the inputs and the slab count alone.  Whatever a launch writes -- weights, the coefficient, slabs, partial
// sums -- is read by later launches only; inside the apply kernel every element is read and written by the same lane.
// LDS: a fixed region and ONE net's rows of all layers (ranenv_ppo.hip's plan): actor and critic rows do not fit side by side, so the
// actor pass runs the actor's forward twice per tile -- once for the action, once more (bit-identical) behind the critics for its own
// backward pass -- and carries only [32][S] of d(-Q/n)/da, the actions (registers) and the row sums across.
#include "ranenv_ppo_parts.hpp"

namespace {

constexpr unsigned SAC_TAG = 0x53414300u;               // the target's Philox draws (ranenv_policy.hip), + position
constexpr unsigned SAC_ACTOR_TAG = 0x53415000u;         // "SAP\0": the actor pass's, + position
constexpr int SAC_FIXED = 5120;           // bytes of LDS in front of the rows: 256 reduction slots | dQ/da [32][16] | target [32] | pick [32]
constexpr int SAC_PARTIALS = 8;           // doubles per slab: sum (Q1 - y)^2, (Q2 - y)^2, Q1, Q2, y | alpha logp - min Q, logp, logp + target entropy
static_assert(SAC_FIXED >= 256 * 8 + NET_ROWS * 16 * 4 + NET_ROWS * 4 + NET_ROWS * 4, "the fixed LDS region holds the slots, dQ/da, the targets and the picks");

// The critics' input rows [x | action] of the tile -> `dst` (zeros beyond the input and beyond the minibatch): the observation from
// `x` [n][10 S], the action columns from at(k) for the thread's pair k (position tid + 256 k of the [32][S] block)
template <class F>
__device__ __forceinline__ void sac_q_rows(const PolicyNet &q, const float *x, long long row0, long long n, int S, float *dst, int tid, F at)
{
    const int ld0 = net_ld(q.kp[0]);
    load_dense_rows(x, row0, n, 10 * S, 10 * S, q.kp[0], 10 * S, 11 * S, dst, tid);
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const int i = tid + 256 * k;
        if (i < NET_ROWS * S) dst[(i / S) * ld0 + 10 * S + (i % S)] = at(k, i / S, i % S);
    }
}

// The squashed-Gaussian epilogue of the thread's pair (row r, position j) on the actor's output rows `o` (stride ld): the draw under
// `tag`, the action and the position's term of log pi (ranenv_sac_targets' expressions, include/ranenv.h)
struct SacDraw { double ls, z, a; bool free; };
__device__ __forceinline__ SacDraw sac_draw(const float *o, int ld, int S, int r, int j, long long i, unsigned tag, unsigned long long seed, unsigned long long draw)
{
    const double raw = (double)o[r * ld + S + j];
    SacDraw d;
    d.ls = clamp_log_std(raw);
    d.free = raw >= -20.0 && raw <= 2.0;
    unsigned w[4];
    philox4x32_10((unsigned)i, (unsigned)((unsigned long long)i >> 32), (unsigned)draw, tag + (unsigned)j, (unsigned)seed, (unsigned)(seed >> 32), w);
    d.z = box_muller(w);
    d.a = tanh(gauss_sample((double)o[r * ld + j], d.ls, d.z));
    return d;
}
__device__ __forceinline__ double sac_logp_term(const SacDraw &d) { return ((((-0.5 * d.z) * d.z - d.ls) - HALF_LN_2PI)) - log((1.0 - d.a * d.a) + 1e-6); }

// dL/d(input) of one tile through `net`: `out` = the output layer's rows, holding dL/d(output); the layers' inputs lie in front of it.
// ppo_backward's dZ' step alone (ppo_dz_blocks) -- no dW, no db -- carried through EVERY layer, layer 0 included, in place over the
// layers' input rows; of layer 0 only the 16-column blocks that hold columns [c0, c1).  Rows are independent.
// Ends behind a barrier: the input rows' columns [c0, c1) hold the gradient.
__device__ __forceinline__ void sac_input_grad(const PolicyNet &net, const float *w, float *out, int tid, int c0, int c1)
{
    float *dz = out;
    for (int l = net.n_layers - 1; l >= 0; l--) {
        float *a = dz - NET_ROWS * net_ld(net.kp[l]);
        ppo_dz_blocks(net, l, w + net.w_off[l], dz, a, l == 0 ? c0 >> 4 : 0, l == 0 ? (c1 + 15) >> 4 : net.kp[l] >> 4, tid);
        __syncthreads();
        dz = a;
    }
}

// The workgroup's sums (threads 0..31 hold `K` each, rows of all its tiles) -> partial[at .. at + K): thread k adds the 32 in thread order
template <int K>
__device__ __forceinline__ void sac_partials(double *red, const double (&st)[K], double *partial, int tid)
{
    __syncthreads();
    if (tid < NET_ROWS)
#pragma unroll
        for (int k = 0; k < K; k++) red[tid * K + k] = st[k];
    __syncthreads();
    if (tid < K) {
        double s = 0.0;
#pragma unroll 1
        for (int r = 0; r < NET_ROWS; r++) s += red[r * K + tid];
        partial[tid] = s;
    }
}

// ---- the critic pass ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) ranenv_sac_critic_kernel(SacPassArgs A)
{
    extern __shared__ float lds[];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int S = A.S;
    const long long n = A.n;
    double *red = (double *)lds;
    float *tgt = lds + (256 * 8 + NET_ROWS * 16 * 4) / 4;
    float *act = lds + SAC_FIXED / 4;
    const int tiles = (int)((n + NET_ROWS - 1) / NET_ROWS);
    const double alpha = exp((double)A.log_ent_coef[0]);
    float *slab = A.slab + (size_t)blockIdx.x * (size_t)A.slab_stride;
    const PolicyNet &actor = A.actor.net;
    double sq0 = 0.0, sq1 = 0.0, sv0 = 0.0, sv1 = 0.0, sy = 0.0;      // (threads 0..31: the sums over the rows they own)

#pragma unroll 1
    for (int tile = (int)blockIdx.x; tile < tiles; tile += (int)gridDim.x) {
        const long long row0 = (long long)tile * NET_ROWS;
        __syncthreads();                       // (the previous tile's backward pass has read its rows)
        // ---- the target: ranenv_sac_target_kernel's steps on next_obs, under the actor and the target critics ------------------
        float *cur = act, *nxt = act + NET_ROWS * net_ld(actor.kp[0]);
        load_dense_rows(A.next_obs, row0, n, 10 * S, actor.in_dim, actor.kp[0], 0, 0, cur, tid);
        __syncthreads();
        net_layers<false, true>(actor, A.actor.w, cur, nxt, lane, wave);
        const int ld = net_ld(actor.np[actor.n_layers - 1]);
        double *term = (double *)act;          // (over the input rows, which nobody reads again)
        float a32[2] = {0.0f, 0.0f};
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const int i = tid + 256 * k;
            if (i >= NET_ROWS * S) continue;
            const int r = i / S, j = i - r * S;
            if (row0 + r >= n) continue;
            const SacDraw d = sac_draw(cur, ld, S, r, j, A.first_row + row0 + r, SAC_TAG, A.seed, A.draw);
            a32[k] = (float)d.a;
            term[i] = sac_logp_term(d);
        }
        __syncthreads();
        const bool own = tid < NET_ROWS && row0 + tid < n;
        double lp = 0.0;
        if (own)
            for (int j = 0; j < S; j++) lp += term[tid * S + j];
        __syncthreads();                       // (the terms are read: the critics' rows overwrite them)
        float v0 = 0.0f, v1 = 0.0f;
#pragma unroll 1
        for (int k = 0; k < 2; k++) {
            const PolicyNet &q = A.qt[k].net;
            cur = act; nxt = act + NET_ROWS * net_ld(q.kp[0]);
            sac_q_rows(q, A.next_obs, row0, n, S, cur, tid, [&](int kk, int, int) { return a32[kk]; });
            __syncthreads();
            net_layers<false, true>(q, A.qt[k].w, cur, nxt, lane, wave);
            if (own) {
                const float vk = cur[tid * net_ld(q.np[q.n_layers - 1])];
                if (k == 0) v0 = vk;
                else v1 = vk;
            }
            // (the next rows land in front of the output rows just read; the layers behind them start behind a barrier)
        }
        if (own) {
            const double nd = A.done[row0 + tid] ? 0.0 : 1.0;
            const float y = (float)((double)A.reward[row0 + tid] + nd * (A.gamma * (fmin((double)v0, (double)v1) - alpha * lp)));
            tgt[tid] = y;
            if (A.target) A.target[row0 + tid] = y;
            sy += (double)y;
        }
        // ---- the live critics on [obs | action]: dL/dQ = (Q - y) / n, the backward pass into the slab --------------------------------
#pragma unroll 1
        for (int k = 0; k < 2; k++) {
            const PolicyNet &q = A.q[k].net;
            __syncthreads();                   // (the net in front has read its rows)
            cur = act; nxt = act + NET_ROWS * net_ld(q.kp[0]);
            sac_q_rows(q, A.obs, row0, n, S, cur, tid, [&](int, int r, int j) { return row0 + r < n ? A.action[(size_t)(row0 + r) * S + j] : 0.0f; });
            __syncthreads();
            net_layers<false, true>(q, A.q[k].w, cur, nxt, lane, wave);
            if (tid < NET_ROWS) {
                float *o = cur + tid * net_ld(q.np[q.n_layers - 1]);
                if (!own) o[0] = 0.0f;
                else {
                    const double d = (double)o[0] - (double)tgt[tid];
                    if (k == 0) { sq0 += d * d; sv0 += (double)o[0]; }
                    else { sq1 += d * d; sv1 += (double)o[0]; }
                    o[0] = (float)(d / (double)n);
                }
            }
            __syncthreads();
            ppo_backward(q, A.q[k].w, slab + A.off[1 + k], cur, tid);
        }
    }
    const double st[5] = {sq0, sq1, sv0, sv1, sy};
    sac_partials<5>(red, st, A.partial + (size_t)blockIdx.x * SAC_PARTIALS, tid);
}

// ---- the actor pass -----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) ranenv_sac_actor_kernel(SacPassArgs A)
{
    extern __shared__ float lds[];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int S = A.S;
    const long long n = A.n;
    double *red = (double *)lds;
    float *dqda = lds + 256 * 8 / 4;          // [32][16]: d(-min Q / n)/da of the tile's rows
    int *pick = (int *)(lds + (256 * 8 + NET_ROWS * 16 * 4 + NET_ROWS * 4) / 4);
    float *act = lds + SAC_FIXED / 4;
    const int tiles = (int)((n + NET_ROWS - 1) / NET_ROWS);
    const double alpha = exp((double)A.log_ent_coef[0]), wrow = 1.0 / (double)n;
    const float wq = (float)(-1.0 / (double)n);
    float *slab = A.slab + (size_t)blockIdx.x * (size_t)A.slab_stride;
    const PolicyNet &actor = A.actor.net;
    const int ld = net_ld(actor.np[actor.n_layers - 1]);
    double s_pi = 0.0, s_lp = 0.0, s_ent = 0.0;

#pragma unroll 1
    for (int tile = (int)blockIdx.x; tile < tiles; tile += (int)gridDim.x) {
        const long long row0 = (long long)tile * NET_ROWS;
        __syncthreads();                       // (the previous tile's backward pass has read its rows)
        // ---- 1. the actor on obs: the action and log pi ---------------------------------------------------------------------------
        float *cur = act, *nxt = act + NET_ROWS * net_ld(actor.kp[0]);
        load_dense_rows(A.obs, row0, n, 10 * S, actor.in_dim, actor.kp[0], 0, 0, cur, tid);
        __syncthreads();
        net_layers<false, true>(actor, A.actor.w, cur, nxt, lane, wave);
        double *term = (double *)act;
        float a32[2] = {0.0f, 0.0f};
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const int i = tid + 256 * k;
            if (i >= NET_ROWS * S) continue;
            const int r = i / S, j = i - r * S;
            if (row0 + r >= n) continue;
            const SacDraw d = sac_draw(cur, ld, S, r, j, A.first_row + row0 + r, SAC_ACTOR_TAG, A.seed, A.draw);
            a32[k] = (float)d.a;
            term[i] = sac_logp_term(d);
        }
        __syncthreads();
        const bool own = tid < NET_ROWS && row0 + tid < n;
        double lp = 0.0;
        if (own)
            for (int j = 0; j < S; j++) lp += term[tid * S + j];
        __syncthreads();                       // (the terms are read: the critics' rows overwrite them)
        // ---- 2. both live critics on [obs | a32]; d(-Q / n)/da of the smaller one (a tie: Q1) ----------------------------------------
        float v0 = 0.0f, v1 = 0.0f;
#pragma unroll 1
        for (int k = 0; k < 2; k++) {
            const PolicyNet &q = A.q[k].net;
            const int ld0 = net_ld(q.kp[0]);
            cur = act; nxt = act + NET_ROWS * ld0;
            sac_q_rows(q, A.obs, row0, n, S, cur, tid, [&](int kk, int, int) { return a32[kk]; });
            __syncthreads();
            net_layers<false, true>(q, A.q[k].w, cur, nxt, lane, wave);
            if (tid < NET_ROWS) {
                float *o = cur + tid * net_ld(q.np[q.n_layers - 1]);
                if (own && k == 0) v0 = o[0];
                if (own && k == 1) v1 = o[0];
                o[0] = own ? wq : 0.0f;
                if (k == 1) pick[tid] = v1 < v0 ? 1 : 0;
            }
            __syncthreads();
            sac_input_grad(q, A.q[k].w, cur, tid, 10 * S, 11 * S);
#pragma unroll
            for (int kk = 0; kk < 2; kk++) {
                const int i = tid + 256 * kk;
                if (i >= NET_ROWS * S) continue;
                const int r = i / S, j = i - r * S;
                if (k == 0 || pick[r]) dqda[r * 16 + j] = act[r * ld0 + 10 * S + j];
            }
            __syncthreads();                   // (the input rows are read: the next rows overwrite them)
        }
        if (own) {
            s_pi += alpha * lp - (double)(v1 < v0 ? v1 : v0);
            s_lp += lp;
            s_ent += lp + A.target_entropy;
        }
        // ---- 3. the actor's forward once more (the same bits), the gradient at its outputs, its backward pass ----------------------
        cur = act; nxt = act + NET_ROWS * net_ld(actor.kp[0]);
        load_dense_rows(A.obs, row0, n, 10 * S, actor.in_dim, actor.kp[0], 0, 0, cur, tid);
        __syncthreads();
        net_layers<false, true>(actor, A.actor.w, cur, nxt, lane, wave);
        float gm[2] = {0.0f, 0.0f}, gl[2] = {0.0f, 0.0f};
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const int i = tid + 256 * k;
            if (i >= NET_ROWS * S) continue;
            const int r = i / S, j = i - r * S;
            if (row0 + r >= n) continue;
            const SacDraw d = sac_draw(cur, ld, S, r, j, A.first_row + row0 + r, SAC_ACTOR_TAG, A.seed, A.draw);
            // u = mu + exp(ls) z, a = tanh(u):  d logp / du = 2 a (1 - a^2) / ((1 - a^2) + 1e-6),  da / du = 1 - a^2
            const double one = 1.0 - d.a * d.a;
            const double du = (wrow * alpha) * (((2.0 * d.a) * one) / (one + 1e-6)) + (double)dqda[r * 16 + j] * one;
            gm[k] = (float)du;
            gl[k] = d.free ? (float)(du * (exp(d.ls) * d.z) - wrow * alpha) : 0.0f;
        }
        __syncthreads();                       // (every pair has read its outputs: they are overwritten)
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const int i = tid + 256 * k;
            if (i >= NET_ROWS * S) continue;
            const int r = i / S, j = i - r * S;
            cur[r * ld + j] = gm[k];
            cur[r * ld + S + j] = gl[k];
        }
        __syncthreads();
        ppo_backward(actor, A.actor.w, slab + A.off[0], cur, tid);
    }
    const double st[3] = {s_pi, s_lp, s_ent};
    sac_partials<3>(red, st, A.partial + (size_t)blockIdx.x * SAC_PARTIALS + 5, tid);
}

// ---- apply: the used slabs summed, Adam, polyak; the step's second apply also steps the coefficient and writes the statistics ---------
__global__ void __launch_bounds__(256) ranenv_sac_apply_kernel(SacApplyArgs A)
{
    const SacApplySeg &s = A.seg[blockIdx.y];
    const long long e = (long long)blockIdx.x * 256 + (long long)threadIdx.x;
    if (e < s.floats) {
        if (s.op & SAC_OP_ADAM) {
            float *p = A.slab + s.slab_off + e;
            float g = *p;
            *p = 0.0f;
#pragma unroll 1
            for (int u = 1; u < A.used; u++) {
                p += A.slab_stride;
                g = g + *p;
                *p = 0.0f;
            }
            if (s.grad) s.grad[e] = g;
            adam_elem(s.w[e], s.m[e], s.v[e], g, adam_step(A.lr, 0.9, 0.999, 1e-8, s.t));
        }
        if (s.op & SAC_OP_POLYAK) {
            const float omt = (float)(1.0 - A.tau), tf = (float)A.tau;
            s.tgt[e] = omt * s.tgt[e] + tf * s.w[e];
        }
    }
    if (!A.last || blockIdx.x != 0 || blockIdx.y != 0 || threadIdx.x != 0) return;
    double p[SAC_PARTIALS];
#pragma unroll
    for (int k = 0; k < SAC_PARTIALS; k++) p[k] = 0.0;
#pragma unroll 1
    for (int u = 0; u < A.used; u++)
#pragma unroll
        for (int k = 0; k < SAC_PARTIALS; k++) p[k] += A.partial[(size_t)u * SAC_PARTIALS + k];
    const double n = (double)A.n;
    const float lec = A.ent[0];
    const double mean_e = p[7] / n;
    double *out = A.stats;
    out[0] = 0.5 * (p[0] / n + p[1] / n); out[1] = p[5] / n; out[2] = A.auto_coef ? -((double)lec * mean_e) : 0.0; out[3] = exp((double)lec);
    out[4] = p[6] / n; out[5] = p[2] / n; out[6] = p[3] / n; out[7] = p[4] / n;
    float g = 0.0f;
    if (A.auto_coef) {
        g = (float)(-mean_e);
        adam_elem(A.ent[0], A.ent[1], A.ent[2], g, adam_step(A.lr, 0.9, 0.999, 1e-8, A.t_ent));
    }
    if (A.grad_ent) A.grad_ent[0] = g;
#pragma unroll
    for (int k = 0; k < 4; k++) A.dev_t[k] = A.t_new[k];
}

}  // namespace

namespace ranenv_dev {

size_t sac_lds_bytes(const PolicyNet &actor, const PolicyNet &critic)
{
    const int x = ppo_act_floats(actor), y = ppo_act_floats(critic);
    return (size_t)SAC_FIXED + sizeof(float) * (size_t)(x > y ? x : y);
}

hipError_t launch_sac_pass(hipStream_t s, int which, int grid, size_t lds, const SacPassArgs &a)
{
    return which == 0 ? launch_lds<ranenv_sac_critic_kernel>(dim3((unsigned)grid), dim3(256), lds, s, a) : launch_lds<ranenv_sac_actor_kernel>(dim3((unsigned)grid), dim3(256), lds, s, a);
}

hipError_t launch_sac_apply(hipStream_t s, const SacApplyArgs &a)
{
    long long most = 1;
    for (int k = 0; k < a.n_seg; k++) most = a.seg[k].floats > most ? a.seg[k].floats : most;
    hipLaunchKernelGGL(ranenv_sac_apply_kernel, dim3((unsigned)((most + 255) / 256), (unsigned)a.n_seg), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace ranenv_dev
