// ranenv_aux.hip -- the small kernels of libranenv_hip.so and their launch functions (ranenv_internal.h, "launch table").
#include "ranenv_numeric.hpp"

namespace {

// Sort the envs by the waves a compact step of theirs needs: class c = ceil(slice members of the env's scenario / 64) - 1.
// ONE workgroup (the counts are built in LDS: no memset in front, one launch in all).  `flag`: a device word that
// ranenv_advance_kernel sets when an env has restarted -- without `force` the kernel does nothing unless the word is set, and it
// clears it: an auto-reset loop in which no episode ended pays one empty launch, not a re-sort (and no host read-back of `done`).
__global__ void __launch_bounds__(1024) ranenv_persist_classify_kernel(const ranenv_episode *eps, const int32_t *members, int B, int n_class,
                                                                       int one_class, int32_t *list, int32_t *count, int *flag, int force)
{
    __shared__ int cnt[CORE_NT / WAVE];
    if (!force && *flag == 0) return;                 // (uniform: every thread reads the word before thread 0 clears it, behind the barriers)
    if (threadIdx.x < CORE_NT / WAVE) cnt[threadIdx.x] = 0;
    __syncthreads();
    for (int e = (int)threadIdx.x; e < B; e += (int)blockDim.x) {
        const int m = members[eps[e].scenario];
        int c = m <= 0 ? 0 : (m + WAVE - 1) / WAVE - 1;
        c = c < n_class ? c : n_class - 1;
        if (one_class) c = n_class - 1;           // a batch far below what the chip holds: idle waves cost nothing, a second launch does
        const int pos = atomicAdd(&cnt[c], 1);
        list[(size_t)c * B + pos] = e;
    }
    __syncthreads();
    if ((int)threadIdx.x < n_class) count[threadIdx.x] = cnt[threadIdx.x];
    if (threadIdx.x == 0) *flag = 0;
}

// ---------------------------------------------------------------------------------------------
// Sidecars of the SE pool for the gather mode, built once per bound pool (ranenv_set_se_mode):
//   mean[tile][u]    = np.mean(SE[u, :]) in float64, numpy's pairwise order (row_sums' `full`, divided by R): bit for bit what
//                      the streaming kernel derives from the tile every TTI
//   um[tile][u][Rp]  = the tile UE-major, rows padded with zeros to Rp = R rounded up to 8 floats
// One workgroup per tile, thread = UE for the means; the copy is a plain index transform (reads served by L2).
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(CORE_NT) ranenv_se_sidecar_kernel(const float *pool, long long stride, long long tile0, int U, int R, int Rp,
                                                                    int quad, double *mean, float *um)
{
    const long long t = tile0 + blockIdx.x;
    const float *tile = pool + (size_t)t * (size_t)stride;
    const int tid = threadIdx.x;
    const int u = tid < U ? tid : U - 1;
    SeStream<4> se;
    se.init(tile, U, u, R, quad != 0);
    double full = 0.0, part = 0.0;
    row_sums(se, R, [](int) { return false; }, full, part, []() {});
    if (tid < U) mean[(size_t)t * U + tid] = full / (double)R;
    float *out = um + (size_t)t * (size_t)U * Rp;
    for (int i = tid; i < U * Rp; i += (int)blockDim.x) {
        const int uu = i / Rp, r = i - uu * Rp;
        out[i] = r < R ? (quad ? tile[((size_t)(r >> 2) * U + uu) * 4 + (r & 3)] : tile[(size_t)r * U + uu]) : 0.0f;
    }
}

// RB-major [n][R][U] -> RB-quad-major [n][ceil(R/4)][U][4] (ranenv_se_retile_quad): one float4 of the output per thread, zeros behind RB R-1
__global__ void __launch_bounds__(256) ranenv_se_retile_quad_kernel(const float *src, float *dst, long long n_quads, int U, int R)
{
    const int Rq = (R + 3) >> 2;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_quads; i += (long long)gridDim.x * blockDim.x) {
        const long long t = i / ((long long)Rq * U);
        const int rem = (int)(i - t * (long long)Rq * U), qr = rem / U, u = rem - qr * U;
        const float *tile = src + (size_t)t * (size_t)U * R;
        se_v4f v;
        v.x = tile[(size_t)(4 * qr) * U + u];
        v.y = 4 * qr + 1 < R ? tile[(size_t)(4 * qr + 1) * U + u] : 0.0f;
        v.z = 4 * qr + 2 < R ? tile[(size_t)(4 * qr + 2) * U + u] : 0.0f;
        v.w = 4 * qr + 3 < R ? tile[(size_t)(4 * qr + 3) * U + u] : 0.0f;
        ((se_v4f *)dst)[i] = v;
    }
}

// RB-major [n][R][U] or RB-quad-major [n][ceil(R/4)][U][4] (tiles `stride` floats apart) -> member lines [n][U][lines][32]
// (ranenv_se_retile_member_lines; the layout: ranenv_numeric.hpp, "Member lines"): one float4 of the output per thread -- the 16 bytes
// lane j of a cluster loads --, +0.0 wherever the layout pads.
// packed_f4 > 0 (ranenv_se_retile_member_lines_packed; the handle's copy): a tile of the output is packed_f4 float4s -- the
// whole-group lines [U][lines - 1][32], the tail block [U][8] (UE u's last R mod 8 RBs at the head of its 32-byte slot) and +0.0 up
// to the stride; a row without a tail has no block and is laid out as above.
__global__ void __launch_bounds__(256) ranenv_se_retile_member_lines_kernel(const float *src, long long stride, int quad, float *dst, long long n_f4,
                                                                            int U, int R, const MemberLineTable tb, long long packed_f4)
{
    const int nlw = packed_f4 > 0 && tb.tail > 0 ? tb.lines - 1 : tb.lines;          // lines per UE in front of the block
    const long long per_tile = packed_f4 > 0 ? packed_f4 : (long long)U * tb.lines * 8;
    const int walk_f4 = U * nlw * 8;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_f4; i += (long long)gridDim.x * blockDim.x) {
        const long long t = i / per_tile;
        const int rem = (int)(i - t * per_tile);
        const float *tile = src + (size_t)t * (size_t)stride;
        float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (rem < walk_f4) {
            const int u = rem / (nlw * 8), rl = rem - u * (nlw * 8), l = rl >> 3, j = rl & 7;
            auto at = [&](int r) { return quad ? tile[((size_t)(r >> 2) * U + u) * 4 + (r & 3)] : tile[(size_t)r * U + u]; };
            const int rb0 = tb.rb0[l], ng = tb.groups[l];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (ng > 0) v[k] = k < ng ? at(rb0 + 8 * k + j) : 0.0f;          // position 4 j + k: group k of the chunk, accumulator j
                else v[k] = 4 * j + k < tb.tail ? at(rb0 + 4 * j + k) : 0.0f;     // the tail line: position = RB
            }
        } else if (rem < walk_f4 + 2 * U && nlw < tb.lines) {
            const int q = rem - walk_f4, u = q >> 1, p0 = (q & 1) * 4, rb0 = R - tb.tail;      // the block: slot u, its first or second 16 bytes
            auto at = [&](int r) { return quad ? tile[((size_t)(r >> 2) * U + u) * 4 + (r & 3)] : tile[(size_t)r * U + u]; };
#pragma unroll
            for (int k = 0; k < 4; k++) v[k] = p0 + k < tb.tail ? at(rb0 + p0 + k) : 0.0f;
        }
        se_v4f o; o.x = v[0]; o.y = v[1]; o.z = v[2]; o.w = v[3];
        ((se_v4f *)dst)[i] = o;
    }
}

// ---------------------------------------------------------------------------------------------
// Per-tile statistics of the SE pool (ranenv_build_se_stats): what the scenario load figures read of a tile
// (results/gen_results.py:260-497, :1251-1451), per UE over its R RBs, in float64 on the float32 values:
//   stats[tile][0][u] = np.mean  -- row_sums' `full` / R: the gather sidecar's row_mean bit for bit
//   stats[tile][1][u] = np.std   -- sqrt(pairwise_sum((x - mean) * (x - mean)) / R), population (ddof = 0): the same leaves over the squares
//   stats[tile][2][u], [3][u] = np.min, np.max (the quad layout's padding behind RB R-1 is never shown to them)
// The sidecar kernel's launch shape: one workgroup per tile, thread = UE; stat-major rows, so a wave stores whole lines.  The
// deviations need the mean first: the row is walked twice, and the second walk re-reads what this workgroup has just pulled
// through L2 (plain loads: SeStream<4> carries no non-temporal bit).  Plain / and sqrt: correctly rounded in this build.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(CORE_NT) ranenv_se_tile_stats_kernel(const float *pool, long long stride, long long tile0, int U, int R, int quad,
                                                                       double *stats)
{
    const long long t = tile0 + blockIdx.x;
    const float *tile = pool + (size_t)t * (size_t)stride;
    const int tid = threadIdx.x;
    const int u = tid < U ? tid : U - 1;
    SeStream<4> se;
    se.init(tile, U, u, R, quad != 0);
    double sum = 0.0, none = 0.0;
    float lo = __builtin_inff(), hi = -__builtin_inff();
    row_sums(se, R, RowNoPart(), sum, none, []() {}, 1.0, RowIdentity(), [&](float x) { lo = x < lo ? x : lo; hi = x > hi ? x : hi; });
    const double mean = sum / (double)R;
    se.init(tile, U, u, R, quad != 0);
    double sq = 0.0;
    row_sums(se, R, RowNoPart(), sq, none, []() {}, 1.0, [mean](double d) { const double e = d - mean; return e * e; });
    if (tid < U) {
        double *out = stats + (size_t)t * 4 * (size_t)U + tid;
        out[0] = mean; out[(size_t)U] = sqrt(sq / (double)R); out[2 * (size_t)U] = (double)lo; out[3 * (size_t)U] = (double)hi;
    }
}

// Gather-only ingest (ranenv_bind_se_gather_from_power): the same two sidecars straight from QuaDRiGa received power
// (channels/quadriga.py:56-69), without an RB-major float32 pool ever existing.  The float32 SE of an element is what
// ranenv_se_from_power would have stored; the mean runs through row_sums over those float32 values, so both sidecars are bit for
// bit what ranenv_set_se_mode builds from the pool ranenv_se_from_power writes.
struct PowerStream {           // row_sums' source interface over a tile of float64 power, converted on the way in
    static constexpr int NSLOT = 2;
    const double *tile; int U, u, R; double tx, noise;
    float q[NSLOT][8];
    DEVFN float se_of(int r) const
    {
        const int rr = r < R ? r : R - 1;                              // (padding rows of the last group: never summed)
        return (float)log2(1.0 + (tx * tile[(size_t)rr * U + u]) / (0.0 + noise));
    }
    DEVFN void refill(int d, int r0) {
#pragma unroll
        for (int j = 0; j < 8; j++) q[d][j] = se_of(r0 + j);
    }
    DEVFN void init() { for (int d = 0; d < NSLOT; d++) if (d * 8 < R) refill(d, d * 8); }
    DEVFN void take(int d, float (&x)[8], int) {
#pragma unroll
        for (int j = 0; j < 8; j++) x[j] = q[d][j];
    }
};

__global__ void __launch_bounds__(CORE_NT) ranenv_se_sidecar_from_power_kernel(const double *power, long long tile0, int U, int R, int Rp,
                                                                               double tx, double noise, double *mean, float *um)
{
    const long long t = tile0 + blockIdx.x;
    const double *tile = power + (size_t)t * (size_t)U * (size_t)R;
    const int tid = threadIdx.x;
    PowerStream ps;
    ps.tile = tile; ps.U = U; ps.u = tid < U ? tid : U - 1; ps.R = R; ps.tx = tx; ps.noise = noise;
    ps.init();
    double full = 0.0, part = 0.0;
    row_sums(ps, R, [](int) { return false; }, full, part, []() {});
    if (tid < U) mean[(size_t)t * U + tid] = full / (double)R;
    float *out = um + (size_t)t * (size_t)U * Rp;
    for (int i = tid; i < U * Rp; i += (int)blockDim.x) {
        const int uu = i / Rp, r = i - uu * Rp;
        out[i] = r < R ? (float)log2(1.0 + (tx * tile[(size_t)r * U + uu]) / (0.0 + noise)) : 0.0f;
    }
}

// =============================================================================================
// Alternative heads: the observation of SchedTWC / SchedColORAN (agents/sched_twc.py:165-346:
// 3 requirements + 7 slice means per slice, slices in index order, metric-major) and their rewards
// (sched_twc.py:348-413, sched_colran.py:348-419), from the state the core kernel just wrote.
// One workgroup = one env, thread = slot (slice, UE position), launched after the core kernel when
// head outputs are bound.
//
// These agents push every raw observation twice into their 10-deep deque (sched_twc.py:174-177), so
// their window is the last D/2 TTIs counted twice, and "the previous entry" is the current TTI again:
// entry i of their deque is TTI i/2 of the window ring.
// =============================================================================================
struct SharedHead {
    double rows[GRP][10][GRP];    // per slice: mean SE, served Mbps, effective Mbps, occupancy, latency, loss,
                                  //            raw capacity, drift x3 -- by UE position, zero padded
    double sv[GRP][3];            // slice drift means (-2: not declared)
    double thr_raw[GRP], occ_m[GRP];
    int nues[GRP];
    double terms[3 * GRP], nw[3 * GRP];   // the reward's terms and weights (one lane fills them: LDS, not 784 B of scratch per lane)
};

// numpy pairwise_sum of n <= 128 doubles by one lane: a leaf of its recursion over elements a(0) .. a(n - 1)
template <typename Elem>
DEVFN double np_leaf(Elem a, int n)
{
    if (n < 8) { double r = 0.0; for (int i = 0; i < n; i++) r += a(i); return r; }
    double r[8];
    for (int j = 0; j < 8; j++) r[j] = a(j);
    int i = 8;
    for (; i < n - (n % 8); i += 8) for (int j = 0; j < 8; j++) r[j] += a(i + j);
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; i++) res += a(i);
    return res;
}
DEVFN double np_sum_seq(const double *a, int n) { return np_leaf([a](int i) { return a[i]; }, n); }

// numpy pairwise_sum of any n by one lane: above 128 elements numpy halves the range at a multiple of 8 and adds the two halves'
// sums, left + right.  The recursion is walked with an explicit stack of frames in LDS (`stack`: PW_DEPTH frames of this lane's own;
// a kernel that recursed would need scratch): a range of 2^31 elements is 25 frames deep.
struct PwFrame { int off, n, right_next; double left; };
enum { PW_DEPTH = 26 };
template <typename Elem>
DEVFN double np_pairwise(Elem a, int n, PwFrame *stack)
{
    int top = 0;
    stack[0].off = 0; stack[0].n = n; stack[0].right_next = 0;
    for (;;) {
        const int off = stack[top].off, len = stack[top].n;
        if (len > 128) {                           // descend into the left half
            int h = len / 2; h -= h % 8;
            stack[top + 1].off = off; stack[top + 1].n = h; stack[top + 1].right_next = 0;
            top += 1;
            continue;
        }
        double v = np_leaf([&](int i) { return a(off + i); }, len);
        for (;;) {                                 // hand the finished range's sum to its parent
            if (top == 0) return v;
            top -= 1;
            if (!stack[top].right_next) {          // it was the left half: keep it, walk the right half
                int h = stack[top].n / 2; h -= h % 8;
                stack[top].left = v; stack[top].right_next = 1;
                stack[top + 1].off = stack[top].off + h; stack[top + 1].n = stack[top].n - h; stack[top + 1].right_next = 0;
                top += 1;
                break;
            }
            v = stack[top].left + v;
        }
    }
}

__global__ void __launch_bounds__(CORE_NT) ranenv_head_kernel(const KP p, double *head_acc, int reset)
{
    __shared__ SharedHead sh;
    auto wave_sync = []() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); };
    const int e = p.e0 + blockIdx.x, tid = threadIdx.x;
    if (p.env_mask != nullptr && p.env_mask[e] == 0) return;
    if (head_acc && reset && tid == 0) { head_acc[(size_t)e * 2 + 0] = 0.0; head_acc[(size_t)e * 2 + 1] = 0.0; }   // a new episode's sums
    const int S = p.S, U = p.U, D = p.D;
    const int sc = __builtin_amdgcn_readfirstlane(p.episodes[e].scenario);
    const int hlen = __builtin_amdgcn_readfirstlane(ST_hist_len(p)[e]);      // counters after this TTI's push
    const int npush = __builtin_amdgcn_readfirstlane(ST_n_push(p)[e]);
    const int s = tid / GRP, pos = tid % GRP;
    const bool in_grid = s < S;
    const int NS16 = S * GRP;
    int ue = -1, mp = 1;
    if (tid < NS16) { const size_t ts = (size_t)sc * NS16 + tid; ue = TB_slot_ue(p)[ts]; mp = TB_slot_mp(p)[ts]; }
    const bool have = ue >= 0;
    const int gsh = (tid & 63) & ~(GRP - 1);
    const int n = __popc((unsigned)((__ballot(have) >> gsh) & 0xffffull));
    int active = 0, has_req = 0, bsize = 1, blat = 1, msg = 1, npar = 0;
    int pm[3] = {0, 0, 0}, po[3] = {0, 0, 0};
    double pv[3] = {0.0, 0.0, 0.0}, traffic_tab = 0.0;
    if (in_grid) {
        const size_t row = (size_t)sc * S + s;
        const int32_t *si = TB_slice_i32(p) + row * 8;
        active = si[0]; has_req = si[1]; bsize = si[3]; blat = si[4]; msg = si[5]; npar = si[6];
        traffic_tab = TB_slice_f64(p)[row * 2 + 1];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            pm[k] = TB_param_i32(p)[(row * 3 + k) * 2 + 0];
            po[k] = TB_param_i32(p)[(row * 3 + k) * 2 + 1];
            pv[k] = TB_param_f64(p)[row * 3 + k];
        }
    }
    // ---- the UE of this slot ----------------------------------------------------------------------
    double vals[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (have) {
        const size_t su = (size_t)e * U + ue;
        const int total = ST_queue_pkts(p)[su];
        const long long sum_age = ST_queue_age_sum(p)[su];
        const double sem = ST_se_mean(p)[su];
        const double sent = (double)ST_pkt_effective_thr(p)[su], thr = (double)ST_pkt_throughputs(p)[su];
        // the heads' window: deque entry i is TTI i/2; view_len = min(2*hlen, D)
        const int vlen = 2 * hlen < D ? 2 * hlen : D;
        double sw = 0.0, dw = 0.0;
        for (int j = 0; 2 * j < vlen; j++) {
            int idx = npush - 1 - j; idx += idx < 0 ? D : 0;
            const double mult = 2 * j + 1 < vlen ? 2.0 : 1.0;
            sw += mult * (double)ST_ring_sent(p)[((size_t)e * D + idx) * U + ue];
            dw += mult * (double)ST_ring_drop(p)[((size_t)e * D + idx) * U + ue];
        }
        const double occ = (double)total / (double)mp;
        const double lat = total > 0 ? (double)sum_age / (double)total : 0.0;
        const double bp = occ * (double)bsize + dw + sw;                     // common.py:32-53
        const double loss = bp != 0.0 ? dw / bp : 0.0;
        vals[0] = sem;
        vals[1] = thr * (double)msg / 1e6;                                   // sched_twc.py:255-266
        vals[2] = sent * (double)msg / 1e6;                                  // :269-280
        vals[3] = occ; vals[4] = lat; vals[5] = loss; vals[6] = thr;
        if (has_req) {                                                       // common.py:68-340, heads' deque
            const double o = p.over;
#pragma unroll
            for (int qi = 0; qi < 3; qi++) {
                if (qi < npar) {
                    const int metric = pm[qi], op = po[qi];
                    const double value = pv[qi];
                    double res;
                    if (metric == RANENV_METRIC_THROUGHPUT) {
                        double x = (sent * (double)msg) / 1e6;
                        if (d_isclose(occ, 0.0)) x = value * (1.1 + o);      // entry 1 of their deque = this TTI
                        if (d_apply_op(op, x, value)) res = (x > value * (1.0 + o)) ? 1.0 : (x - value) / (value * o);
                        else res = -((value - x) / value);
                    } else if (metric == RANENV_METRIC_RELIABILITY) {
                        const double x = loss;
                        const double band = (100.0 - value) / 100.0;
                        if (d_apply_op(op, 100.0 * (1.0 - x), value)) res = (x < band * (1.0 - o)) ? 1.0 : (band - x) / (band * o);
                        else res = -((x - band) / (value / 100.0));
                    } else {
                        const double x = lat;
                        if (d_apply_op(op, x, value)) res = (x < value * (1.0 - o)) ? 1.0 : (value - x) / (value * o);
                        else res = -((x - value) / ((double)blat - value));
                    }
                    vals[7] = metric == 0 ? res : vals[7]; vals[8] = metric == 1 ? res : vals[8]; vals[9] = metric == 2 ? res : vals[9];
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 10; k++) sh.rows[s][k][pos] = vals[k];
    wave_sync();
    // ---- the slice (lane 0 of its 16 writes) -------------------------------------------------------
    if (in_grid && pos == 0) {
        float *o = p.head_obs ? p.head_obs + (size_t)e * 10 * S : nullptr;
        double m[7] = {0, 0, 0, 0, 0, 0, 0};
        if (n > 0) {
#pragma unroll
            for (int k = 0; k < 7; k++) m[k] = np_sum16_lds(sh.rows[s][k], n) / (double)n;
        }
        double sv[3] = {-2.0, -2.0, -2.0};
        double req[3] = {0.0, 0.0, 0.0};
        if (n > 0 && has_req) {
#pragma unroll
            for (int qi = 0; qi < 3; qi++) {
                if (qi < npar) {
                    const int mt = pm[qi];
                    const double mean = np_sum16_lds(sh.rows[s][7 + mt], n) / (double)n;
                    sv[0] = mt == 0 ? mean : sv[0]; sv[1] = mt == 1 ? mean : sv[1]; sv[2] = mt == 2 ? mean : sv[2];
                    // requirements = [reliability, latency, throughput]            sched_twc.py:216-226
                    req[0] = mt == RANENV_METRIC_RELIABILITY ? pv[qi] : req[0];
                    req[1] = mt == RANENV_METRIC_LATENCY ? pv[qi] : req[1];
                    req[2] = mt == RANENV_METRIC_THROUGHPUT ? pv[qi] : req[2];
                }
            }
        }
        if (o) {
            o[3 * s + 0] = (float)req[0]; o[3 * s + 1] = (float)req[1]; o[3 * s + 2] = (float)req[2];
#pragma unroll
            for (int k = 0; k < 6; k++) o[(3 + k) * S + s] = (float)m[k];
            o[9 * S + s] = (float)(d_isclose((double)active, 1.0) ? traffic_tab : 0.0);  // :325-337
        }
        sh.sv[s][0] = sv[0]; sh.sv[s][1] = sv[1]; sh.sv[s][2] = sv[2];
        sh.thr_raw[s] = m[6]; sh.occ_m[s] = m[3];
        sh.nues[s] = n;
    }
    __syncthreads();
    // ---- the rewards (one lane; a few dozen values) ------------------------------------------------
    if (tid == 0 && p.head_reward) {
        double *terms = sh.terms, *nw = sh.nw;
        int q = 0;
        double r_col = 0.0;
        for (int sl = 0; sl < S; sl++) {
            const int nu = sh.nues[sl];
            if (nu == 0) continue;                                               // sched_twc.py:364-365
            const size_t row = (size_t)sc * S + sl;
            const double w = TB_slice_f64(p)[row * 2 + 0] != 0.0 ? 2.0 : 1.0;    // :382-391
            for (int k = 0; k < 3; k++) {
                const double v = sh.sv[sl][k];
                if (d_isclose(v, -2.0) || !(v < 0.0)) continue;                  // :376-378, :395-399
                terms[q] = v; nw[q] = w; q++;
            }
            const int32_t *si = TB_slice_i32(p) + row * 8;
            if (si[0] != 0) {                                                    // sched_colran.py:372-419
                const int uc = TB_slice_usecase(p)[row];
                const double pkt = (double)si[5];
                if (uc & 1) r_col += ((sh.thr_raw[sl] * pkt) / 1e6) / 200.0;
                if (uc & 2) r_col -= ((sh.occ_m[sl] * (double)si[3]) * pkt / 1e6) / 2000.0;
            }
        }
        const double wsum = np_sum_seq(nw, q);
        double r_twc = 0.0;
        if (!d_isclose(wsum, 0.0)) {
            for (int i = 0; i < q; i++) terms[i] = terms[i] * nw[i] / wsum;
            r_twc = np_sum_seq(terms, q);
        }
        p.head_reward[(size_t)e * 2 + 0] = r_twc;
        p.head_reward[(size_t)e * 2 + 1] = r_col;
        if (head_acc && !reset) {      // episode sums of the two head rewards: one add per TTI, in TTI order
            head_acc[(size_t)e * 2 + 0] += r_twc;
            head_acc[(size_t)e * 2 + 1] += r_col;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Per-slice episode metrics (ranenv_enable_slice_metrics; the columns are spelled out in include/ranenv.h): what the paper's
// per-slice figures read per TTI (results/gen_results.py:874-970, :791-809, :1007-1018), kept as running sums per (env, slice).
// Launched behind the step kernel for the same envs on the same stream and restates nothing of it: the minimum declared drift is
// the step's reward[e][s + 1], the per-metric drifts and their declared flags are its obs_intra[e][s][0..5], the packet counts its
// raw per-UE outputs.  One workgroup = one env, thread = slot (slice in INDEX order, UE position), as the head kernel; the four
// packet sums run over a slice's 16 lanes on one DPP row.  Lane k < 10 of a slice owns column k: one writer per cell and TTI,
// TTIs in stream order, so the sums do not depend on the launch path.  reset != 0: the launch follows a reset and zeroes the rows
// of the envs under the mask.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(CORE_NT) ranenv_slice_metrics_kernel(const KP p, double *slice_acc, int reset)
{
    const int e = p.e0 + blockIdx.x, tid = threadIdx.x;
    if (p.env_mask != nullptr && p.env_mask[e] == 0) return;
    const int S = p.S, U = p.U;
    const int s = tid / GRP, pos = tid % GRP;
    if (s >= S) return;                                    // (whole rows of 16 lanes leave: the DPP sums below stay inside a row)
    double *cell = slice_acc + ((size_t)e * S + s) * RANENV_SLICE_METRIC_COLS + pos;
    if (reset) { if (pos < RANENV_SLICE_METRIC_COLS) *cell = 0.0; return; }
    const int sc = __builtin_amdgcn_readfirstlane(p.episodes[e].scenario);
    const int ue = TB_slot_ue(p)[(size_t)sc * S * GRP + tid];
    int inc = 0, cap = 0, sent = 0, drop = 0;
    if (ue >= 0) {
        const size_t su = (size_t)e * U + ue;
        inc = ST_pkt_incoming(p)[su]; cap = ST_pkt_throughputs(p)[su]; sent = ST_pkt_effective_thr(p)[su]; drop = ST_dropped_pkts(p)[su];
    }
    inc = row16_sum(inc); cap = row16_sum(cap); sent = row16_sum(sent); drop = row16_sum(drop);
    const bool active = TB_slice_i32(p)[((size_t)sc * S + s) * 8 + 0] != 0;
    const double dmin = p.reward[(size_t)e * (S + 1) + s + 1];                 // minimum over the declared metrics (0.0: none declared)
    const float *oa = p.obs_intra + ((size_t)e * S + s) * (size_t)(2 * p.Us + 9);
    double add;
    if (pos >= 6) add = (double)(pos == 6 ? inc : (pos == 7 ? cap : (pos == 8 ? sent : drop)));
    else if (!active) add = 0.0;                           // an inactive slice may have UEs, a request and a drift: it counts nowhere
    else if (pos == 0) add = 1.0;
    else if (pos == 1) add = dmin < 0.0 ? 1.0 : 0.0;
    else if (pos == 5) add = dmin < 0.0 ? dmin : 0.0;
    else add = (oa[pos + 1] > 0.0f && oa[pos - 2] < 0.0f) ? 1.0 : 0.0;       // metric pos - 2: declared flag [3 + m], drift [m]
    if (pos < RANENV_SLICE_METRIC_COLS) *cell += add;
}

// ---------------------------------------------------------------------------------------------
// Device traces (ranenv_bind_trace; the row is spelled out in include/ranenv.h): one row of the caller's ring per recorded env and
// TTI, a pure copy of what the step just left.  Launched behind the step (and head) kernel for the recorded envs of the launch's
// range, in front of whatever follows an episode end: the env's row still holds the finished episode's descriptor, the step's done
// flag and the terminal observation.  One workgroup = one recorded env; it owns the env's column and its two counters (one launch
// per env and TTI, TTIs in stream order: no atomics).  The tile is 4 R U bytes of a row's 4 R U + 36 U + 4 S (2 Us + 9) + 57 S + 21: it
// is split across the whole workgroup, lane = UE fastest, so that every store instruction writes consecutive floats of one RB row
// -- from an RB-major source (the pool, or the call's explicit tile) a linear copy, from an RB-quad-major pool one 16-byte load
// per (quad, UE) and up to four stores, one into each of the quad's RB rows (the pad RBs behind R - 1 are dropped).  The position
// of the tile is the one the step read: the counter it left behind, minus one.  A full ring: the row is counted as lost, nothing
// is written.
// ---------------------------------------------------------------------------------------------
// The pool tile env e's last step read: ST_se_pos is where its NEXT step reads, so one behind it, around the trace's end
DEVFN size_t trace_tile_no(const KP &p, int e)
{
    const ranenv_episode ep = p.episodes[e];
    int pos = ST_se_pos(p)[e];
    pos = (pos < 1 || pos > ep.se_len ? ep.se_len : pos) - 1;
    return (size_t)(ep.se_base + (long long)(pos < 0 ? 0 : pos));
}

__global__ void __launch_bounds__(CORE_NT) ranenv_trace_kernel(const KP p, const TraceArgs a)
{
    const int i = a.first + (int)blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const int e = __builtin_amdgcn_readfirstlane(a.env[i]), col = __builtin_amdgcn_readfirstlane(a.slot[i]);
    const int row = __builtin_amdgcn_readfirstlane(a.count[col]);
    const ranenv_trace &o = a.out;
    if (row >= o.capacity || row < 0) {
        if (tid == 0) a.lost[col] += 1;
        return;
    }
    const int S = p.S, U = p.U, R = p.R, W = 2 * p.Us + 9;
    const size_t at = (size_t)row * (size_t)o.n_envs + (size_t)col;      // this row's index in every buffer
    for (int u = tid; u < U; u += nt) {
        const size_t su = (size_t)e * U + u, du = at * U + u;
        if (o.pkt_incoming) o.pkt_incoming[du] = ST_pkt_incoming(p)[su];
        if (o.pkt_throughputs) o.pkt_throughputs[du] = ST_pkt_throughputs(p)[su];
        if (o.pkt_effective_thr) o.pkt_effective_thr[du] = ST_pkt_effective_thr(p)[su];
        if (o.dropped_pkts) o.dropped_pkts[du] = ST_dropped_pkts(p)[su];
        if (o.queue_pkts) o.queue_pkts[du] = ST_queue_pkts(p)[su];
        if (o.rb_start) o.rb_start[du] = ST_rb_start(p)[su];
        if (o.rb_count) o.rb_count[du] = ST_rb_count(p)[su];
        if (o.queue_age_sum) o.queue_age_sum[du] = ST_queue_age_sum(p)[su];
    }
    if (o.se) {
        float *dst = o.se + at * (size_t)R * U;
        if (p.se_tiles != nullptr || !a.se_quad) {
            const float *src;
            if (p.se_tiles != nullptr) src = p.se_tiles + (size_t)e * U * R;
            else src = a.se_pool + trace_tile_no(p, e) * (size_t)a.se_stride;
            for (int k = tid; k < R * U; k += nt) dst[k] = src[k];
        } else {
            const se_v4f *src = (const se_v4f *)(a.se_pool + trace_tile_no(p, e) * (size_t)a.se_stride);
            const int Rq = (R + 3) >> 2;
            for (int k = tid; k < Rq * U; k += nt) {                     // k = quad * U + UE
                const int q = k / U, u = k - q * U, r = 4 * q;
                const se_v4f v = src[k];
                float *d = dst + (size_t)r * U + u;
                d[0] = v.x;
                if (r + 1 < R) d[(size_t)U] = v.y;
                if (r + 2 < R) d[2 * (size_t)U] = v.z;
                if (r + 3 < R) d[3 * (size_t)U] = v.w;
            }
        }
    }
    if (o.reward) for (int k = tid; k <= S; k += nt) o.reward[at * (S + 1) + k] = p.reward[(size_t)e * (S + 1) + k];
    if (o.scores) for (int k = tid; k < S; k += nt) o.scores[at * S + k] = ST_policy_scores(p)[(size_t)e * S + k];
    if (o.intra)
        for (int k = tid; k < S; k += nt) {                              // what intra_alloc took for slice k
            int c = p.fixed_intra;
            if (c == RANENV_INTRA_PER_SLICE) c = p.intra ? (int)p.intra[(size_t)e * S + k] : RANENV_INTRA_RR;
            o.intra[at * S + k] = (uint8_t)c;
        }
    if (o.obs_inter) for (int k = tid; k < 10 * S; k += nt) o.obs_inter[at * 10 * S + k] = p.obs_inter[(size_t)e * 10 * S + k];
    if (o.obs_intra) for (int k = tid; k < S * W; k += nt) o.obs_intra[at * S * W + k] = p.obs_intra[(size_t)e * S * W + k];
    const int step_new = ST_step_no(p)[e];
    if (tid == 0) {
        if (o.step_number) o.step_number[at] = step_new - 1;
        if (o.episode_number) o.episode_number[at] = ST_episode_no(p)[e];
        if (o.scenario) o.scenario[at] = p.episodes[e].scenario;
        const int max_steps_e = p.max_steps_env ? p.max_steps_env[e] : p.max_steps;
        if (o.done) o.done[at] = p.done ? p.done[e] : (uint8_t)(step_new >= max_steps_e ? 1 : 0);
    }
    __syncthreads();                       // every wave has formed its addresses from `row` before it moves on
    if (tid == 0) a.count[col] = row + 1;
}

// ---------------------------------------------------------------------------------------------
// Scenario load (ranenv_rbs_needed; the columns are spelled out in include/ranenv.h): the RBs a slice would need to serve its
// intent's traffic and its capacity per RB (results/gen_results.py:277-497, :1251-1451), from the tile statistics and the scenario
// row alone -- no env is stepped.  One workgroup = one (episode, step); thread u holds UE u's four statistics.  Lane 6 s + k then adds
// row k (mean, mean - std, mean + std, min, max, the membership itself) times slice s's membership over ALL U entries, the zeros in
// place, in numpy's pairwise order (np.sum(x * slice_ues, axis=1)); lane s makes slice s's divisions, three lanes add the slices up
// in index order.  Small and cold: ~100 lanes walk an LDS row each.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(CORE_NT) ranenv_rbs_needed_kernel(const RbsArgs a)
{
    __shared__ double rows[5][CORE_NT];
    __shared__ int slc[CORE_NT];
    __shared__ double sums[GRP][6], need[GRP][3];
    __shared__ PwFrame stack[6 * GRP][3];             // U <= 256: one split at most
    const int tid = threadIdx.x, S = a.S, U = a.U;
    const int ei = (int)(blockIdx.x / (unsigned)a.n_steps), t = (int)(blockIdx.x - (unsigned)ei * (unsigned)a.n_steps);
    const ranenv_episode ep = a.eps[ei];
    const double *st = a.stats + (size_t)se_tile_of(ep, t) * 4 * (size_t)U;
    if (tid < U) {
        const double mean = st[tid], sd = st[(size_t)U + tid];
        rows[0][tid] = mean; rows[1][tid] = mean - sd; rows[2][tid] = mean + sd;
        rows[3][tid] = st[2 * (size_t)U + tid]; rows[4][tid] = st[3 * (size_t)U + tid];
        slc[tid] = a.ue_slice[(size_t)ep.scenario * U + tid];
    }
    __syncthreads();
    if (tid < 6 * S) {
        const int s = tid / 6, k = tid - 6 * s;
        const double *row = rows[k < 5 ? k : 0];
        sums[s][k] = np_pairwise([&](int i) { const double m = slc[i] == s ? 1.0 : 0.0; return k < 5 ? row[i] * m : m; }, U, stack[tid]);
    }
    __syncthreads();
    if (tid < S) {
        const int s = tid;
        const size_t trow = (size_t)ep.scenario * S + s;
        const double den = sums[s][5], R = (double)a.R;
        const bool some = den != 0.0;
        const double avg_se = some ? sums[s][0] / den : 0.0, min_se = some ? sums[s][1] / den : 0.0, max_se = some ? sums[s][2] / den : 0.0;
        const double thr = a.slice_i32[trow * 8 + 1] != 0 ? a.slice_f64[trow * 2 + 1] : 0.0;
        const double per_rb = a.bw_mhz / R, want = thr * den;
        const double avg_n = avg_se > 0.0 ? want / (per_rb * avg_se) : 0.0;
        const double min_n = max_se > 0.0 ? want / (per_rb * max_se) : 0.0;
        double max_n = min_se > 0.0 ? want / (per_rb * min_se) : 0.0;       // (not R where the low SE is not positive: the reference's rule)
        max_n = max_n > R ? R : max_n;                                      // the only column that is clipped, per slice
        need[s][0] = avg_n; need[s][1] = min_n; need[s][2] = max_n;
        if (a.slice_out) {
            double *o = a.slice_out + ((size_t)blockIdx.x * S + s) * RANENV_LOAD_SLICE_COLS;
            o[0] = avg_n; o[1] = min_n; o[2] = max_n;
            o[3] = some ? (sums[s][0] * a.bw_mhz) / (den * R) : 0.0;
            o[4] = some ? (sums[s][3] * a.bw_mhz) / (den * R) : 0.0;
            o[5] = some ? (sums[s][4] * a.bw_mhz) / (den * R) : 0.0;
        }
    }
    __syncthreads();
    if (tid < 3) {
        double r = need[0][tid];
        for (int s = 1; s < S; s++) r = r + need[s][tid];
        a.net_out[(size_t)blockIdx.x * 3 + tid] = r;
    }
}

// np.mean over an episode's T network rows, per column: numpy's pairwise recursion over T, divided by T (np.mean's bits up to T = 8192,
// where numpy starts adding up buffer-sized blocks).  One workgroup per episode.
__global__ void __launch_bounds__(WAVE) ranenv_rbs_episode_mean_kernel(const double *net, int n_steps, double *episode_mean)
{
    __shared__ PwFrame stack[3][PW_DEPTH];
    const int tid = threadIdx.x;
    if (tid >= 3) return;
    const double *col = net + (size_t)blockIdx.x * (size_t)n_steps * 3 + tid;
    const double sum = np_pairwise([col](int i) { return col[(size_t)i * 3]; }, n_steps, stack[tid]);
    episode_mean[(size_t)blockIdx.x * 3 + tid] = sum / (double)n_steps;
}

// ---------------------------------------------------------------------------------------------
// Channel ingest: received power -> spectral efficiency (channels/quadriga.py:56-69), elementwise.
// 8 B read + 4 B written per element; two elements per thread and grid-stride, 16-byte loads.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) ranenv_se_from_power_kernel(const double *power, float *se, long long n,
                                                                   double tx_per_rb, double noise)
{
    const long long stride = (long long)gridDim.x * blockDim.x * 2;
    for (long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 2; i < n; i += stride) {
        if (i + 1 < n && ((size_t)(power + i) & 15) == 0 && ((size_t)(se + i) & 7) == 0) {
            const double2 g = *reinterpret_cast<const double2 *>(power + i);
            float2 o;
            o.x = (float)log2(1.0 + (tx_per_rb * g.x) / (0.0 + noise));
            o.y = (float)log2(1.0 + (tx_per_rb * g.y) / (0.0 + noise));
            *reinterpret_cast<float2 *>(se + i) = o;
        } else {
            se[i] = (float)log2(1.0 + (tx_per_rb * power[i]) / (0.0 + noise));
            if (i + 1 < n) se[i + 1] = (float)log2(1.0 + (tx_per_rb * power[i + 1]) / (0.0 + noise));
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Auto-reset, part 1 (part 2 is the step kernel in RESET mode under the mask written here): one workgroup
// per env.  For an env whose episode just ended (done != 0): keep its terminal observation, pick the next
// episode number -- sequential from `initial`, or random in [initial, max) (simu.py:361,377,546; the draw is
// counter-based: seed, env id, resets so far) -- and install that episode's descriptor from the table.
// ---------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(64) ranenv_advance_kernel(const AdvanceArgs a)
{
    const int e = a.e0 + blockIdx.x, tid = threadIdx.x;
    const bool d = a.done[e] != 0;
    if (tid == 0) a.mask[e] = d ? 1 : 0;
    if (!d) return;
    if (a.acc) {          // the finished episode's sums go to the env's log (the reset that follows zeroes the running sums)
        const int n = a.ep_n[e];                  // read by every thread of this one wave before thread 8 stores
        if (tid < 8 && n < a.ep_slots) a.ep_acc[((size_t)e * a.ep_slots + n) * 8 + tid] = a.acc[(size_t)e * 8 + tid];
        if (a.head_acc && tid >= 16 && tid < 18 && n < a.ep_slots) a.head_ep_acc[((size_t)e * a.ep_slots + n) * 2 + (tid - 16)] = a.head_acc[(size_t)e * 2 + (tid - 16)];
        if (a.slice_acc && n < a.ep_slots) {      // ... and its per-slice block, with the scenario row it was played on (the slice index means another slice type in every scenario)
            for (int i = tid; i < a.n_slice; i += 64) a.slice_ep_acc[((size_t)e * a.ep_slots + n) * a.n_slice + i] = a.slice_acc[(size_t)e * a.n_slice + i];
            if (tid == 9) a.slice_ep_scenario[(size_t)e * a.ep_slots + n] = a.episodes[e].scenario;      // (thread 0 installs the next descriptor below)
        }
        if (tid == 8) a.ep_n[e] = n + 1;
    }
    if (a.term_inter) for (int i = tid; i < a.n_inter; i += 64) a.term_inter[(size_t)e * a.n_inter + i] = a.obs_inter[(size_t)e * a.n_inter + i];
    if (a.term_intra) for (int i = tid; i < a.n_intra; i += 64) a.term_intra[(size_t)e * a.n_intra + i] = a.obs_intra[(size_t)e * a.n_intra + i];
    if (a.term_head && a.head_obs) for (int i = tid; i < a.n_head; i += 64) a.term_head[(size_t)e * a.n_head + i] = a.head_obs[(size_t)e * a.n_head + i];
    if (tid == 0) {
        const int cur = a.episode_no[e], cnt = a.reset_count[e] + 1;
        int next;
        if (a.random) {
            unsigned rnd[4];
            philox4x32_10((unsigned)(a.env_id_base + e), (unsigned)cnt, 0x45504953u /* "EPIS" */, 0u,
                          (unsigned)a.seed, (unsigned)(a.seed >> 32), rnd);
            next = a.initial + (int)(rnd[0] % (unsigned)(a.max_ep - a.initial));
        } else {
            next = cur + 1 < a.max_ep ? cur + 1 : a.initial;
        }
        a.episode_no[e] = next; a.reset_count[e] = cnt;
        a.episodes[e] = a.table[next - a.table_first];
        if (a.cls_flag) *a.cls_flag = 1;
    }
}

// ---------------------------------------------------------------------------------------------
// Do the traffic traces carry bits for UEs outside every slice?  (MultSliceTraffic.step never does: it draws for the UEs
// of slices with a request only, traffics/mult_slice.py:24-32.)  One workgroup per episode descriptor scans the rows of
// its traffic trace at the idle UEs of its scenario.  Only when none does may a step leave idle UEs alone (KP::compact).
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) ranenv_idle_traffic_kernel(const ranenv_episode *eps, const int32_t *pool, int U,
                                                                  const int32_t *lane_slice, const int32_t *lane_ue, int *violations)
{
    const ranenv_episode ep = eps[blockIdx.x];
    int bad = 0;
    for (int l = threadIdx.x; l < U; l += (int)blockDim.x) {
        const size_t tu = (size_t)ep.scenario * U + l;
        if (lane_slice[tu] >= 0) continue;
        const int ue = lane_ue[tu];
        for (int row = 0; row < ep.trf_len; row++) bad |= pool[((size_t)ep.trf_base + (size_t)row) * U + ue] != 0;
    }
    if (bad) atomicOr(violations, 1);
}

// ddiv() against the compiler's IEEE division on caller-supplied operands (ranenv_selftest_ddiv: the parity check of the guard-free
// sequence inside the shipped build -- no second build with RANENV_FAST_DIV=0 needed)
__global__ void __launch_bounds__(256) ranenv_ddiv_selftest_kernel(const double *a, const double *b, double *fast, double *ieee, long long n)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        fast[i] = ddiv(a[i], b[i]);
        ieee[i] = a[i] / b[i];
    }
}

// ---------------------------------------------------------------------------------------------
// Generalised advantage estimation over a recorded trajectory (ranenv_collect / ranenv_gae; the arithmetic is spelled out in
// include/ranenv.h).  Lane = (env, column): every [t] slice is read as contiguous lines.  The recurrence is a chain of n_steps
// dependent float64 multiplies and adds per lane; slot t - 1's reward / value / done do not depend on it and are requested before
// slot t's step of the chain is evaluated.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) ranenv_gae_kernel(int n_steps, int B, int n_cols, const double *reward, int reward_stride, const float *vf,
                                                         const uint8_t *done, double gamma, double lambda, float *adv, float *vtarg)
{
    const long long n = (long long)B * n_cols, i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long long b = i / n_cols;
    // the reward of (t, env, column): rows of reward_stride doubles per env (= n_cols: packed, as ranenv_gae's; ranenv_collect_head
    // reads one column of the [T][B][2] head rewards)
    const long long rn = (long long)B * reward_stride, ri = b * reward_stride + (i - b * n_cols);
    const double gl = gamma * lambda;
    double a_next = 0.0, v1 = (double)vf[(long long)n_steps * n + i];
    double r = reward[(long long)(n_steps - 1) * rn + ri], v0 = (double)vf[(long long)(n_steps - 1) * n + i];
    uint8_t d = done[(long long)(n_steps - 1) * B + b];
    for (int t = n_steps - 1; t >= 0; t--) {
        double rp = 0.0, vp = 0.0;
        uint8_t dp = 0;
        if (t > 0) { rp = reward[(long long)(t - 1) * rn + ri]; vp = (double)vf[(long long)(t - 1) * n + i]; dp = done[(long long)(t - 1) * B + b]; }
        const double nd = d ? 0.0 : 1.0;
        const double delta = (r + (gamma * v1) * nd) - v0;
        const double a = delta + (gl * nd) * a_next;
        if (adv) adv[(long long)t * n + i] = (float)a;
        if (vtarg) vtarg[(long long)t * n + i] = (float)(a + v0);
        a_next = a; v1 = v0;
        r = rp; v0 = vp; d = dp;
    }
}

// ... under a population's per-member pairs: the lane finds the member that owns its env -- the last m with first[m] <= b, by binary
// search -- once, in front of the T-step chain, then runs ranenv_gae_kernel's chain on that member's (gamma, lambda): the same
// operations in the same order, written out a second time (sharing them through a function reorders ranenv_gae_kernel's instructions)
__global__ void __launch_bounds__(256) ranenv_gae_pop_kernel(int n_steps, int B, int n_cols, const double *reward, int reward_stride, const float *vf,
                                                             const uint8_t *done, GaePop g, float *adv, float *vtarg)
{
    const long long n = (long long)B * n_cols, i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long long b = i / n_cols;
    int lo = 0, hi = g.pop.n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((long long)g.pop.first[mid] <= b) lo = mid;
        else hi = mid;
    }
    const double gamma = g.gamma[lo], lambda = g.lambda[lo];
    const long long rn = (long long)B * reward_stride, ri = b * reward_stride + (i - b * n_cols);
    const double gl = gamma * lambda;
    double a_next = 0.0, v1 = (double)vf[(long long)n_steps * n + i];
    double r = reward[(long long)(n_steps - 1) * rn + ri], v0 = (double)vf[(long long)(n_steps - 1) * n + i];
    uint8_t d = done[(long long)(n_steps - 1) * B + b];
    for (int t = n_steps - 1; t >= 0; t--) {
        double rp = 0.0, vp = 0.0;
        uint8_t dp = 0;
        if (t > 0) { rp = reward[(long long)(t - 1) * rn + ri]; vp = (double)vf[(long long)(t - 1) * n + i]; dp = done[(long long)(t - 1) * B + b]; }
        const double nd = d ? 0.0 : 1.0;
        const double delta = (r + (gamma * v1) * nd) - v0;
        const double a = delta + (gl * nd) * a_next;
        if (adv) adv[(long long)t * n + i] = (float)a;
        if (vtarg) vtarg[(long long)t * n + i] = (float)(a + v0);
        a_next = a; v1 = v0;
        r = rp; v0 = vp; d = dp;
    }
}

// A population role's descriptor table (PolicyNets::tab): entry m0 + i = proto with its packed copy at proto.w + i * stride
__global__ void __launch_bounds__(64) ranenv_net_table_kernel(PolicyNet *tab, int m0, int n, PolicyNet proto, long long stride)
{
    const int i = (int)threadIdx.x;
    if (i >= n) return;
    PolicyNet e = proto;
    e.w = proto.w + (long long)i * stride;
    tab[m0 + i] = e;
}

// ---------------------------------------------------------------------------------------------
// Off-policy collection (ranenv_collect_replay / ranenv_replay_sample; the rules are spelled out in include/ranenv.h).
// ---------------------------------------------------------------------------------------------
// A partition's rows of the head observation / of the actor's scores -> their slot of the replay ring: contiguous ranges of 8-byte words
__global__ void __launch_bounds__(256) ranenv_copy_words_kernel(unsigned long long *dst0, const unsigned long long *src0, long long n0,
                                                                unsigned long long *dst1, const unsigned long long *src1, long long n1)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n0 + n1; i += (long long)gridDim.x * blockDim.x) {
        if (i < n0) dst0[i] = src0[i];
        else dst1[i - n0] = src1[i - n0];
    }
}

// Uniform minibatch: GRP lanes per sampled row.  Lane 0 of the group draws the index once and hands it to the others; an observation
// row is 40 * S bytes -- always a multiple of 8, not always of 16 (S = 5: 200) -- so rows move as 8-byte words.
__global__ void __launch_bounds__(256) ranenv_replay_sample_kernel(const ReplaySampleArgs a)
{
    const int tid = (int)threadIdx.x, l = tid & (GRP - 1);
    const long long i = (long long)blockIdx.x * (256 / GRP) + (tid >> 4);
    if (i >= a.n) return;                              // (a whole group at a time)
    unsigned lo = 0, hi = 0;
    if (l == 0) {
        unsigned o[4];
        philox4x32_10((unsigned)i, (unsigned)((unsigned long long)i >> 32), (unsigned)a.draw, (unsigned)(a.draw >> 32), (unsigned)a.seed,
                      (unsigned)(a.seed >> 32), o);
        const unsigned long long u = ((unsigned long long)o[1] << 32) | o[0];
        const unsigned long long idx = __umul64hi(u, (unsigned long long)a.n_rows);      // floor(u * n_rows / 2^64) < n_rows
        lo = (unsigned)idx; hi = (unsigned)(idx >> 32);
    }
    lo = __shfl(lo, 0, GRP); hi = __shfl(hi, 0, GRP);
    const size_t row = ((size_t)hi << 32) | lo, S = (size_t)a.S, out = (size_t)i;
    const unsigned long long *so = (const unsigned long long *)(a.ring_obs + row * 10 * S), *sn = (const unsigned long long *)(a.ring_next_obs + row * 10 * S);
    unsigned long long *po = (unsigned long long *)(a.obs + out * 10 * S), *pn = (unsigned long long *)(a.next_obs + out * 10 * S);
    for (int w = l; w < 5 * a.S; w += GRP) { po[w] = so[w]; pn[w] = sn[w]; }
    for (int j = l; j < a.S; j += GRP) a.action[out * S + j] = (float)a.ring_action[row * S + j];
    if (l == 0) {
        a.reward[out] = (float)a.ring_reward[row * (size_t)a.reward_cols + a.reward_col];
        a.done[out] = a.ring_done[row];
        if (a.index) a.index[out] = (long long)row;
    }
}

// ---------------------------------------------------------------------------------------------
// A RANENV_NET_BF16 net's weights at bind: f32 W [N][K] -> bf16 [np][kp], round to nearest even (the conversion the policy kernel
// applies to its activations: v_cvt_pk_bf16_f32), zeros in the padding.  A thread owns two neighbouring columns (kp is even).
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) ranenv_pack_bf16_kernel(const float *src, int N, int K, int np, int kp, unsigned *dst)
{
    const long long pairs = (long long)np * (kp / 2);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < pairs; i += (long long)gridDim.x * blockDim.x) {
        const int n = (int)(i / (kp / 2)), k = 2 * (int)(i - (long long)n * (kp / 2));
        const float lo = n < N && k < K ? src[(size_t)n * K + k] : 0.0f, hi = n < N && k + 1 < K ? src[(size_t)n * K + k + 1] : 0.0f;
        typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
        const bf16x2 v = {(__bf16)lo, (__bf16)hi};
        dst[i] = __builtin_bit_cast(unsigned, v);
    }
}

}  // namespace

namespace ranenv_dev {

void launch_pack_bf16(hipStream_t s, const float *src, int N, int K, int np, int kp, unsigned short *dst)
{
    long long blocks = ((long long)np * (kp / 2) + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(ranenv_pack_bf16_kernel, dim3((unsigned)blocks), dim3(256), 0, s, src, N, K, np, kp, (unsigned *)dst);
}

void launch_copy_words(hipStream_t s, unsigned long long *dst0, const unsigned long long *src0, long long n0, unsigned long long *dst1,
                       const unsigned long long *src1, long long n1)
{
    long long blocks = (n0 + n1 + 255) / 256;
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(ranenv_copy_words_kernel, dim3((unsigned)(blocks < 1 ? 1 : blocks)), dim3(256), 0, s, dst0, src0, n0, dst1, src1, n1);
}

void launch_replay_sample(hipStream_t s, const ReplaySampleArgs &a)
{
    const long long per = 256 / GRP;
    hipLaunchKernelGGL(ranenv_replay_sample_kernel, dim3((unsigned)((a.n + per - 1) / per)), dim3(256), 0, s, a);
}

void launch_gae(hipStream_t s, int n_steps, int B, int n_cols, const double *reward, int reward_stride, const float *vf, const uint8_t *done,
                double gamma, double lambda, float *adv, float *vtarg)
{
    const long long n = (long long)B * n_cols;
    hipLaunchKernelGGL(ranenv_gae_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n_steps, B, n_cols, reward, reward_stride, vf, done,
                       gamma, lambda, adv, vtarg);
}

void launch_gae_pop(hipStream_t s, int n_steps, int B, int n_cols, const double *reward, int reward_stride, const float *vf, const uint8_t *done,
                    const GaePop &g, float *adv, float *vtarg)
{
    const long long n = (long long)B * n_cols;
    hipLaunchKernelGGL(ranenv_gae_pop_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n_steps, B, n_cols, reward, reward_stride, vf, done,
                       g, adv, vtarg);
}

void launch_net_table(hipStream_t s, PolicyNet *tab, int m0, int n, const PolicyNet &proto, long long stride)
{
    hipLaunchKernelGGL(ranenv_net_table_kernel, dim3(1), dim3(POP_MAX), 0, s, tab, m0, n, proto, stride);
}

void launch_ddiv_selftest(hipStream_t s, const double *a, const double *b, double *fast, double *ieee, long long n)
{
    long long blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(ranenv_ddiv_selftest_kernel, dim3((unsigned)(blocks < 1 ? 1 : blocks)), dim3(256), 0, s, a, b, fast, ieee, n);
}

void launch_classify(hipStream_t s, const ranenv_episode *eps, const int32_t *members, int B, int n_class, int one_class, int32_t *list,
                     int32_t *count, int *flag, int force)
{
    hipLaunchKernelGGL(ranenv_persist_classify_kernel, dim3(1), dim3(1024), 0, s, eps, members, B, n_class, one_class, list, count, flag, force);
}
void launch_se_sidecar(hipStream_t s, unsigned n_tiles, unsigned block, const float *pool, long long stride, long long tile0, int U, int R, int Rp,
                       int quad, double *mean, float *um)
{
    hipLaunchKernelGGL(ranenv_se_sidecar_kernel, dim3(n_tiles), dim3(block), 0, s, pool, stride, tile0, U, R, Rp, quad, mean, um);
}
void launch_se_tile_stats(hipStream_t s, unsigned n_tiles, unsigned block, const float *pool, long long stride, long long tile0, int U, int R,
                          int quad, double *stats)
{
    hipLaunchKernelGGL(ranenv_se_tile_stats_kernel, dim3(n_tiles), dim3(block), 0, s, pool, stride, tile0, U, R, quad, stats);
}
void launch_rbs_needed(hipStream_t s, unsigned n_episodes, unsigned block, const RbsArgs &a, double *episode_mean)
{
    hipLaunchKernelGGL(ranenv_rbs_needed_kernel, dim3(n_episodes * (unsigned)a.n_steps), dim3(block), 0, s, a);
    hipLaunchKernelGGL(ranenv_rbs_episode_mean_kernel, dim3(n_episodes), dim3(WAVE), 0, s, a.net_out, a.n_steps, episode_mean);
}
void launch_se_sidecar_from_power(hipStream_t s, unsigned n_tiles, unsigned block, const double *power, long long tile0, int U, int R, int Rp,
                                  double tx, double noise, double *mean, float *um)
{
    hipLaunchKernelGGL(ranenv_se_sidecar_from_power_kernel, dim3(n_tiles), dim3(block), 0, s, power, tile0, U, R, Rp, tx, noise, mean, um);
}
void launch_se_retile_quad(hipStream_t s, unsigned blocks, const float *src, float *dst, long long n_quads, int U, int R)
{
    hipLaunchKernelGGL(ranenv_se_retile_quad_kernel, dim3(blocks), dim3(256), 0, s, src, dst, n_quads, U, R);
}
void launch_se_retile_member_lines(hipStream_t s, unsigned blocks, const float *src, long long src_stride, int quad, float *dst, long long n_tiles,
                                   int U, int R, const MemberLineTable &tb, long long packed_f4)
{
    const long long per_tile = packed_f4 > 0 ? packed_f4 : (long long)U * tb.lines * 8;
    hipLaunchKernelGGL(ranenv_se_retile_member_lines_kernel, dim3(blocks), dim3(256), 0, s, src, src_stride, quad, dst, n_tiles * per_tile, U, R, tb, packed_f4);
}
void launch_se_from_power(hipStream_t s, unsigned blocks, const double *power, float *se, long long n, double tx_per_rb, double noise)
{
    hipLaunchKernelGGL(ranenv_se_from_power_kernel, dim3(blocks), dim3(256), 0, s, power, se, n, tx_per_rb, noise);
}
void launch_head(hipStream_t s, dim3 grid, dim3 block, const KP &kp, double *head_acc, int reset)
{
    hipLaunchKernelGGL(ranenv_head_kernel, grid, block, 0, s, kp, head_acc, reset);
}
void launch_slice_metrics(hipStream_t s, dim3 grid, dim3 block, const KP &kp, double *slice_acc, int reset)
{
    hipLaunchKernelGGL(ranenv_slice_metrics_kernel, grid, block, 0, s, kp, slice_acc, reset);
}
void launch_trace(hipStream_t s, unsigned n, const KP &kp, const TraceArgs &a)
{
    hipLaunchKernelGGL(ranenv_trace_kernel, dim3(n), dim3(CORE_NT), 0, s, kp, a);
}
void launch_advance(hipStream_t s, unsigned n_envs, const AdvanceArgs &a) { hipLaunchKernelGGL(ranenv_advance_kernel, dim3(n_envs), dim3(64), 0, s, a); }
void launch_idle_traffic(hipStream_t s, unsigned n_eps, const ranenv_episode *eps, const int32_t *pool, int U, const int32_t *lane_slice,
                         const int32_t *lane_ue, int *violations)
{
    hipLaunchKernelGGL(ranenv_idle_traffic_kernel, dim3(n_eps), dim3(256), 0, s, eps, pool, U, lane_slice, lane_ue, violations);
}

}  // namespace ranenv_dev
