// ranenv_ppo_spread.hip -- the PPO update of ONE agent spread over the chip (ranenv_ppo_bind_spread; include/ranenv.h "One agent over
// the chip").  ranenv_ppo.hip gives a policy pair to one workgroup, which walks every row and passes over every parameter alone; here an
// optimiser step is three launches on the caller's stream, blockIdx.y the kind (0 inter, 1 intra: two independent optimisers, each with
// its own step count -- a kind whose steps are used up returns at once):
//   pass     min(tiles of the minibatch, slabs) workgroups per kind.  Workgroup w walks tiles w, w + grid, ... in ascending order and does
//            per tile what a member's workgroup does (ranenv_ppo.hip) -- the one ppo_tile of ranenv_ppo_parts.hpp on the same LDS plan,
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
// The head policies (ranenv_ppo_bind_head_spread) have three kernels of the same pattern below, on the same elementwise functions.
// Nets per slice (ranenv_ppo_bind_slices_spread) have four kernels of the SAME TEXT: blockIdx.y is one of 1 + S units there, not a kind.
#include "ranenv_ppo_parts.hpp"

namespace {

__device__ __forceinline__ long long spread_floats(const PpoArgs &A, int kind) { return A.net[kind][0].floats + A.net[kind][1].floats; }

// SLICES (ranenv_ppo_bind_slices_spread; "Nets per slice over the chip" below): blockIdx.y is the unit, and what differs is where a
// workgroup finds its work -- spread_unit, at the top of each of the three functions; every other line is the same.
// The unit of this workgroup: its kind, its copy `mem` of the kind's nets, its number `u` among the call's units (counter, statistics,
// gradient block), the first entry `lo` of its share of the lists, and (SLICES alone; else the kind's own P.k[kind] serves) `K`, its
// share of the binding's buffers with its rows and steps
struct SpreadUnit { int kind, mem, u, lo; PpoSpreadKind K; };
template <bool SLICES>
__device__ __forceinline__ void spread_unit(const PpoSpreadArgs &P, const PpoSpreadSlices *X, SpreadUnit &U)
{
    U.u = (int)blockIdx.y;
    if constexpr (!SLICES) { U.kind = U.u; U.mem = 0; U.lo = 0; }
    else {
        const PpoSliceUnit x = ppo_slices_spread_unit(P.a.first, U.u, P.hp.epochs, P.hp.minibatch);
        U.kind = x.kind; U.mem = x.mem; U.lo = x.lo;
        PpoSpreadKind &K = U.K;
        K = P.k[x.kind];
        K.slab += (size_t)x.mem * (size_t)X->slab_unit;
        K.park += (size_t)x.mem * (size_t)X->park_unit;      // (unit 0: mem 0; not wide: park_unit 0 and the pointer is not read)
        K.bpart += (size_t)x.mem * (size_t)X->dbl_unit; K.wstat += (size_t)x.mem * (size_t)X->dbl_unit; K.run += (size_t)x.mem * (size_t)X->dbl_unit;
        K.t0 += x.mem;
        K.n = x.n; K.steps = K.steps ? x.steps : 0;          // (P.k[kind].steps: is the kind trained by this call)
    }
}
// Net k of the unit's kind: where its weights, moments and gradient cell start (SLICES: copy `mem` of the slot, ppo_update_body's rule)
template <bool SLICES>
__device__ __forceinline__ long long spread_at(const PpoArgs &A, int kind, int k, int mem) { return SLICES ? mem * A.net[kind][k].stride : 0; }
template <bool SLICES>
__device__ __forceinline__ PpoSpreadCell spread_cell(const PpoArgs &A, int kind, int mem, long long af, long long e)
{
    PpoSpreadCell c = ppo_spread_cell(A.net[kind][0], A.net[kind][1], af, e);
    if constexpr (SLICES) { const long long at = spread_at<true>(A, kind, e < af ? 0 : 1, mem); c.g += at; c.w += at; c.m += at; c.v += at; }
    return c;
}

template <bool WIDE, bool BF = false, bool SLICES = false>
__device__ __forceinline__ void spread_pass(const PpoSpreadArgs &P, const PpoBf16Net (*bf)[2] = nullptr, const PpoSpreadSlices *X = nullptr)
{
    extern __shared__ float lds[];
    const PpoArgs &A = P.a;
    const ranenv_ppo_hparams &hp = P.hp;
    SpreadUnit U;
    spread_unit<SLICES>(P, X, U);
    const int tid = (int)threadIdx.x, kind = U.kind, mem = U.mem;
    const PpoSpreadKind &K = SLICES ? U.K : P.k[kind];
    if (P.step >= K.steps) return;
    const PpoSpreadStep geo = ppo_spread_step(K.n, hp.minibatch, P.slabs, P.step);
    const int w = (int)blockIdx.x;
    if (w >= geo.grid) return;
    if (P.step == 0 && w == 0 && tid == 0) K.t0[0] = A.t[U.u];
    const int n_nets = A.net[kind][1].net.n_layers > 0 ? 2 : 1;      // net 0 the actor, net 1 the critic

    double *red = (double *)lds, *rowstat = red + 256;
    int *rowidx = (int *)(rowstat + NET_ROWS * PPO_ROW_STATS);
    float *act = lds + PPO_FIXED / 4;
    const int S = A.S, c0 = geo.c0, nb = geo.nb;
    const long long n_record = (long long)A.T * A.B * (kind == 0 ? 1 : S);
    const int32_t *list = A.order[kind] + (size_t)geo.ep * (size_t)A.order_stride[kind] + U.lo;
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
    for (int t0 = w * NET_ROWS; t0 < nb; t0 += geo.grid * NET_ROWS)
        ppo_tile<WIDE, BF>(A, hp, kind, n_nets, list, c0, t0, nb, n_record, wrow, a_mean, a_den, rowstat, rowidx, act, wpark, st, tid,
                           [&](int k) -> const PolicyNet & { return A.net[kind][k].net; },
                           [&](int k) -> const float * { return (BF ? bf[kind][k].acting : A.net[kind][k].w) + spread_at<SLICES>(A, kind, k, mem); },
                           [&](int k) { return slab + (k == 0 ? 0 : A.net[kind][0].floats); }, BF ? bf[kind] : nullptr);
    if (tid == 0) ppo_spread_wstat(K.wstat + (size_t)w * PPO_SPREAD_STATS, st);
}

__global__ void __launch_bounds__(256) ranenv_ppo_spread_pass_kernel(PpoSpreadArgs P) { spread_pass<false>(P); }
__global__ void __launch_bounds__(256) ranenv_ppo_spread_pass_kernel_wide(PpoSpreadArgs P) { spread_pass<true>(P); }

// The reduce and the apply are the elementwise functions of ranenv_ppo_parts.hpp (ppo_spread_*), the head pair's kernels' too
template <bool SLICES = false>
__device__ __forceinline__ void spread_reduce(const PpoSpreadArgs &P, const PpoSpreadSlices *X = nullptr)
{
    __shared__ double red[256];
    const PpoArgs &A = P.a;
    SpreadUnit U;
    spread_unit<SLICES>(P, X, U);
    const int tid = (int)threadIdx.x, kind = U.kind, mem = U.mem;
    const PpoSpreadKind &K = SLICES ? U.K : P.k[kind];
    if (P.step >= K.steps || (int)blockIdx.x >= K.blocks) return;
    const int used = ppo_spread_step(K.n, P.hp.minibatch, P.slabs, P.step).grid;
    const long long af = A.net[kind][0].floats, floats = spread_floats(A, kind);
    const double s = ppo_spread_reduce_elems(K.slab, K.slab_stride, used, floats, tid, [&](long long e) { return spread_cell<SLICES>(A, kind, mem, af, e); });
    const double tot = ppo_sum(red, s, tid);
    if (tid == 0) K.bpart[blockIdx.x] = tot;
}

__global__ void __launch_bounds__(256) ranenv_ppo_spread_reduce_kernel(PpoSpreadArgs P) { spread_reduce(P); }

// stepped(kind, e, w): element e of the kind's packed floats has the new value w (the bf16 binding re-rounds it into the acting copies)
template <bool SLICES = false, class R>
__device__ __forceinline__ void spread_apply(const PpoSpreadArgs &P, R stepped, const PpoSpreadSlices *X = nullptr)
{
    const PpoArgs &A = P.a;
    const ranenv_ppo_hparams &hp = P.hp;
    SpreadUnit U;
    spread_unit<SLICES>(P, X, U);
    const int tid = (int)threadIdx.x, kind = U.kind, mem = U.mem;
    const PpoSpreadKind &K = SLICES ? U.K : P.k[kind];
    if (P.step >= K.steps || (int)blockIdx.x >= K.blocks) return;
    const double norm = sqrt(ppo_spread_norm2(K.bpart, K.blocks));
    const float sc = (float)ppo_clip_scale(hp.grad_clip, norm);
    const int t_call = K.t0[0];
    const AdamStep adam = adam_step(hp.lr, hp.beta1, hp.beta2, hp.eps, t_call + P.step + 1);
    const bool last = P.step == K.steps - 1;
    const long long af = A.net[kind][0].floats, floats = spread_floats(A, kind);
    float *const grad = last && A.grad ? A.grad + (size_t)U.u * (size_t)A.grad_stride : nullptr;
    ppo_spread_apply_elems(floats, grad, sc, adam, tid, [&](long long e) { return spread_cell<SLICES>(A, kind, mem, af, e); },
                           [&](long long e, float w) { stepped(kind, e, w); });
    if (blockIdx.x != 0 || tid != 0) return;
    // ---- block 0: the epoch's statistics and the counter ---------------------------------------------------------------------------
    const PpoSpreadStep geo = ppo_spread_step(K.n, hp.minibatch, P.slabs, P.step);
    ppo_spread_stats(K.run, K.wstat, geo, norm, geo.mb == ppo_spread_per_epoch(K.n, hp.minibatch) - 1,
                     A.stats + ((size_t)U.u * (size_t)A.max_epochs + geo.ep) * RANENV_PPO_STATS, K.n);
    if (last) A.t[U.u] = t_call + K.steps;
}

__global__ void __launch_bounds__(256) ranenv_ppo_spread_apply_kernel(PpoSpreadArgs P) { spread_apply(P, [](int, long long, float) {}); }

// ---- nets per slice over the chip (ranenv_ppo_bind_slices_spread; include/ranenv.h "Nets per slice over the chip") -----------------------
// The per-slice binding's 1 + S policies (ranenv_ppo.hip, SLICES) under the three launches above: blockIdx.y is the unit, every unit an
// optimiser of its own with its own rows, steps, slabs, partials, running sums, t0 cell and counter -- so the rule above holds per
// unit, and a unit whose steps are used up, or whose share is empty, returns at once in all three launches and keeps its bytes.
static_assert(sizeof(PpoSpreadSlicesArgs) <= 4096, "the per-slice spread launches' arguments fit a kernel's argument segment");

__global__ void __launch_bounds__(256) ranenv_ppo_spread_slices_pass_kernel(PpoSpreadSlicesArgs Q) { spread_pass<false, false, true>(Q.p, nullptr, &Q.x); }
__global__ void __launch_bounds__(256) ranenv_ppo_spread_slices_pass_kernel_wide(PpoSpreadSlicesArgs Q) { spread_pass<true, false, true>(Q.p, nullptr, &Q.x); }
__global__ void __launch_bounds__(256) ranenv_ppo_spread_slices_reduce_kernel(PpoSpreadSlicesArgs Q) { spread_reduce<true>(Q.p, &Q.x); }
__global__ void __launch_bounds__(256) ranenv_ppo_spread_slices_apply_kernel(PpoSpreadSlicesArgs Q) { spread_apply<true>(Q.p, [](int, long long, float) {}, &Q.x); }

// ---- bf16 nets over the chip (ranenv_ppo_bind_spread_bfloat; include/ranenv.h "bf16 nets over the chip") ---------------------------------
// The same three launches for RANENV_NET_BF16 nets.  The pass is spread_pass on the bf16 tile (ppo_tile<false, true>): the forward on
// the acting copy as the acting kernels run it, the backward on the bf16 matrix cores (ppo_backward_bf16), the slabs in the F32 packed
// layout.  The reduce is the f32 binding's kernel: PpoNet's g and floats are in that layout.  The apply steps the f32 MASTER copy
// (PpoSpreadCell's w) and stores bf16(master) into the acting copy and the transposed one, a bias into the acting copy's f32 bias: the
// next pass and the next ranenv_collect read trained weights, by launch order alone.
static_assert(sizeof(PpoSpreadBf16Args) <= 4096, "the bf16 spread launches' arguments fit a kernel's argument segment");

__global__ void __launch_bounds__(256) ranenv_ppo_spread_pass_kernel_bf16(PpoSpreadBf16Args Q) { spread_pass<false, true>(Q.p, Q.bf); }

__global__ void __launch_bounds__(256) ranenv_ppo_spread_apply_kernel_bf16(PpoSpreadBf16Args Q)
{
    spread_apply(Q.p, [&](int kind, long long e, float w) {
        const long long af = Q.p.a.net[kind][0].floats;
        const int k = e < af ? 0 : 1;
        ppo_bf16_reround(Q.p.a.net[kind][k].net, Q.bf[kind][k], e - (k ? af : 0), w);
    });
}

// The bind's and a re-bind's seed of one net: element x of the F32 layout's master from the acting copy -- a bf16 weight widened, an
// f32 bias copied -- and, through ppo_bf16_reround (which stores back into the acting copy the value read from it), the transposed copy
__global__ void __launch_bounds__(256) ranenv_ppo_bf16_seed_kernel(PolicyNet net, PpoBf16Net bf, float *master, long long floats)
{
    const long long x = (long long)blockIdx.x * 256 + threadIdx.x;
    if (x >= floats) return;
    float w = 0.0f;
    for (int l = 0; l < net.n_layers; l++) {
        if (x < bf.b_off[l]) { w = (float)((const __bf16 *)(bf.acting + net.w_off[l]))[x - bf.w_off[l]]; break; }
        if (x < bf.b_off[l] + net.np[l]) { w = bf.acting[net.b_off[l] + (x - bf.b_off[l])]; break; }
    }
    master[x] = w;
    ppo_bf16_reround(net, bf, x, w);
}

// ---- the head policies over the chip (ranenv_ppo_bind_head_spread; include/ranenv.h "Head policies over the chip") -------------------
// The same three launches for the head actor, the head critic and log_std [S] on a ranenv_collect_head record: no kinds (a 1-D grid),
// the tile of ranenv_ppo_update_kernel_head (ppo_head_tile), and a third parameter tensor.  Thread j < S of pass workgroup w keeps the
// workgroup's d/d log_std_j in float64 over its tiles and writes it UNROUNDED to gls[w][j]; block 0 of the reduce adds the used slabs'
// in ascending order in float64 and rounds once into ls_g[j] -- where the one-workgroup kernel rounds -- and adds the squares into its
// block partial, so the joint norm covers log_std; block 0 of the apply runs Adam on log_std beside its elements.
// log_std is a weight the previous apply rewrote: the pass loads it into LDS (`lsw`) by lane j at a lane-dependent address, as
// the weight-read rule at ppo_tile asks of every weight; sig[j] = exp(log_std_j) in float64 stands in the reduction slots behind the advantage pass.
__global__ void __launch_bounds__(256) ranenv_ppo_spread_head_pass_kernel(PpoHeadSpreadArgs P)
{
    extern __shared__ float lds[];
    const PpoHeadArgs &A = P.a;
    const ranenv_ppo_hparams &hp = A.hp;
    const PpoHeadSpread &K = P.k;
    const int tid = (int)threadIdx.x, S = A.S;
    const PpoSpreadStep geo = ppo_spread_step(A.n_rows, hp.minibatch, K.slabs, K.step);
    const int w = (int)blockIdx.x;
    if (w >= geo.grid) return;
    if (K.step == 0 && w == 0 && tid == 0) K.t0[0] = A.t[0];

    double *red = (double *)lds, *rowstat = red + 256, *sig = red;
    int *rowidx = (int *)(rowstat + NET_ROWS * PPO_HEAD_ROW_STATS);
    float *lsw = (float *)(rowidx + NET_ROWS);
    float *act = lds + PPO_FIXED / 4;
    const int c0 = geo.c0, nb = geo.nb;
    const long long n_record = (long long)A.T * A.B;
    const int32_t *list = A.order + (size_t)geo.ep * (size_t)A.n_rows;
    const double wrow = 1.0 / (double)nb;
    float *const slab = K.slab + (size_t)w * (size_t)K.slab_stride;
    PpoEpoch st;                               // (thread 0's: this workgroup's tiles)
    if (tid < S) lsw[tid] = A.log_std[tid];

    double g_ls = 0.0;                         // (thread j < S: d/d log_std_j of this workgroup's tiles, rows in order)
    double a_mean = 0.0, a_den = 1.0;
    if (hp.adv_norm)
        ppo_adv_norm(red, nb, tid, [&](int k) {
            const int i = list[c0 + k];
            return i < 0 || i >= n_record ? 0.0 : (double)A.traj.adv[i];
        }, a_mean, a_den);
    if (tid < S) sig[tid] = exp((double)lsw[tid]);      // (thread j reads what thread j wrote; published by the tile loop's first barrier)

#pragma unroll 1
    for (int t0 = w * NET_ROWS; t0 < nb; t0 += geo.grid * NET_ROWS)
        ppo_head_tile(A, list, c0, t0, nb, n_record, wrow, a_mean, a_den, rowstat, rowidx, lsw, sig, act, g_ls, st, tid,
                      [&](int k) { return slab + (k == 0 ? 0 : A.net[0].floats); });
    if (tid < S) K.gls[(size_t)w * S + tid] = g_ls;
    if (tid == 0) ppo_spread_wstat(K.wstat + (size_t)w * PPO_SPREAD_STATS, st);
}

__global__ void __launch_bounds__(256) ranenv_ppo_spread_head_reduce_kernel(PpoHeadSpreadArgs P)
{
    __shared__ double red[256];
    const PpoHeadArgs &A = P.a;
    const PpoHeadSpread &K = P.k;
    const int tid = (int)threadIdx.x, S = A.S;
    const int used = ppo_spread_step(A.n_rows, A.hp.minibatch, K.slabs, K.step).grid;
    const long long af = A.net[0].floats, floats = af + A.net[1].floats;
    double s = ppo_spread_reduce_elems(K.slab, K.slab_stride, used, floats, tid, [&](long long e) { return ppo_spread_cell(A.net[0], A.net[1], af, e); });
    if (blockIdx.x == 0 && tid < S) {          // log_std: the slabs' float64 partials in ascending order, rounded once
        double g = K.gls[tid];
#pragma unroll 1
        for (int u = 1; u < used; u++) g += K.gls[(size_t)u * S + tid];
        const float gf = (float)g;
        A.ls_g[tid] = gf;
        s += (double)gf * (double)gf;
    }
    const double tot = ppo_sum(red, s, tid);
    if (tid == 0) K.bpart[blockIdx.x] = tot;
}

__global__ void __launch_bounds__(256) ranenv_ppo_spread_head_apply_kernel(PpoHeadSpreadArgs P)
{
    const PpoHeadArgs &A = P.a;
    const ranenv_ppo_hparams &hp = A.hp;
    const PpoHeadSpread &K = P.k;
    const int tid = (int)threadIdx.x, S = A.S;
    const double norm = sqrt(ppo_spread_norm2(K.bpart, K.blocks));
    const float sc = (float)ppo_clip_scale(hp.grad_clip, norm);
    const int t_call = K.t0[0];
    const AdamStep adam = adam_step(hp.lr, hp.beta1, hp.beta2, hp.eps, t_call + K.step + 1);
    const bool last = K.step == K.steps - 1;
    const long long af = A.net[0].floats, floats = af + A.net[1].floats;
    float *const grad = last ? A.grad : nullptr;
    ppo_spread_apply_elems(floats, grad, sc, adam, tid, [&](long long e) { return ppo_spread_cell(A.net[0], A.net[1], af, e); });
    if (blockIdx.x != 0) return;
    // ---- block 0: log_std, the epoch's statistics and the counter --------------------------------------------------------------------
    if (tid < S) {
        const float g = A.ls_g[tid];
        if (grad) grad[floats + tid] = g;
        adam_elem(A.log_std[tid], A.ls_m[tid], A.ls_v[tid], g * sc, adam);
    }
    if (tid != 0) return;
    const PpoSpreadStep geo = ppo_spread_step(A.n_rows, hp.minibatch, K.slabs, K.step);
    ppo_spread_stats(K.run, K.wstat, geo, norm, geo.mb == ppo_spread_per_epoch(A.n_rows, hp.minibatch) - 1, A.stats + (size_t)geo.ep * RANENV_PPO_STATS, A.n_rows);
    if (last) A.t[0] = t_call + K.steps;
}

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

hipError_t launch_ppo_spread_slices_step(hipStream_t s, size_t lds, const PpoSpreadSlicesArgs &q, bool wide)
{
    const PpoSpreadArgs &a = q.p;
    int grid = 0, blocks = 0;
    for (int u = 0; u < q.x.n_units; u++) {
        const PpoSliceUnit x = ppo_slices_spread_unit(a.a.first, u, a.hp.epochs, a.hp.minibatch);
        if (!a.k[x.kind].steps || a.step >= x.steps) continue;
        const int g = ppo_spread_step(x.n, a.hp.minibatch, a.slabs, a.step).grid;
        grid = g > grid ? g : grid;
        blocks = a.k[x.kind].blocks > blocks ? a.k[x.kind].blocks : blocks;
    }
    if (grid == 0) return hipSuccess;
    const dim3 pass((unsigned)grid, (unsigned)q.x.n_units), elem((unsigned)blocks, (unsigned)q.x.n_units), block(256);
    const hipError_t e = wide ? launch_lds<ranenv_ppo_spread_slices_pass_kernel_wide>(pass, block, lds, s, q) : launch_lds<ranenv_ppo_spread_slices_pass_kernel>(pass, block, lds, s, q);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ranenv_ppo_spread_slices_reduce_kernel, elem, block, 0, s, q);
    hipLaunchKernelGGL(ranenv_ppo_spread_slices_apply_kernel, elem, block, 0, s, q);
    return hipGetLastError();
}

size_t ppo_bf16_lds_bytes(const PolicyNet &actor, const PolicyNet *critic)
{
    int n = ppo_bf16_act_bytes(actor);
    if (critic && critic->n_layers > 0) { const int v = ppo_bf16_act_bytes(*critic); n = v > n ? v : n; }
    return (size_t)PPO_FIXED + (size_t)n;
}

hipError_t launch_ppo_spread_step_bf16(hipStream_t s, size_t lds, const PpoSpreadBf16Args &q)
{
    const PpoSpreadArgs &a = q.p;
    int grid = 0, blocks = 0;
    for (int k = 0; k < 2; k++) {
        if (a.step >= a.k[k].steps) continue;
        const int g = ppo_spread_step(a.k[k].n, a.hp.minibatch, a.slabs, a.step).grid;
        grid = g > grid ? g : grid;
        blocks = a.k[k].blocks > blocks ? a.k[k].blocks : blocks;
    }
    if (grid == 0) return hipSuccess;
    const dim3 pass((unsigned)grid, 2), elem((unsigned)blocks, 2), block(256);
    const hipError_t e = launch_lds<ranenv_ppo_spread_pass_kernel_bf16>(pass, block, lds, s, q);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ranenv_ppo_spread_reduce_kernel, elem, block, 0, s, a);
    hipLaunchKernelGGL(ranenv_ppo_spread_apply_kernel_bf16, elem, block, 0, s, q);
    return hipGetLastError();
}

hipError_t launch_ppo_bf16_seed(hipStream_t s, const PolicyNet &net, const PpoBf16Net &bf, float *master, long long floats)
{
    hipLaunchKernelGGL(ranenv_ppo_bf16_seed_kernel, dim3((unsigned)((floats + 255) / 256)), dim3(256), 0, s, net, bf, master, floats);
    return hipGetLastError();
}

hipError_t launch_ppo_spread_head_step(hipStream_t s, size_t lds, const PpoHeadSpreadArgs &a)
{
    const int grid = ppo_spread_step(a.a.n_rows, a.a.hp.minibatch, a.k.slabs, a.k.step).grid;
    const dim3 pass((unsigned)grid), elem((unsigned)a.k.blocks), block(256);
    const hipError_t e = launch_lds<ranenv_ppo_spread_head_pass_kernel>(pass, block, lds, s, a);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ranenv_ppo_spread_head_reduce_kernel, elem, block, 0, s, a);
    hipLaunchKernelGGL(ranenv_ppo_spread_head_apply_kernel, elem, block, 0, s, a);
    return hipGetLastError();
}

}  // namespace ranenv_dev
