// ranenv_internal.h -- what the translation units of libranenv_hip.so share: the kernel-argument block (KP) and the structures it
// points to, the slab accessors, and the LAUNCH TABLE -- the functions through which the host side of the ABI (ranenv_host.cpp)
// reaches the kernels, which live in ranenv_step.hip (one object per row width NP, -DRANENV_NP=8 / 10 / 16: they compile in parallel)
// and ranenv_aux.hip (the small kernels: class sort, sidecars, tile statistics, re-tiling, ingest, heads, episode advance, traffic examination,
// scenario load).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <cstddef>
#include <cstdint>

#include "ranenv.h"

#ifndef RANENV_DIAG
#define RANENV_DIAG 0   /* diagnostic builds only (tools/build_variants.sh; see the table in DESIGN.md section 8): 3 / 4 / 7 / 11 skip the UE step / the
                           observation tail / the allocation / the masked half of the stream (tools/valu_phases.sh counts instructions by difference),
                           9 / 12 stamp s_memtime at the phase boundaries of the one-TTI / the persistent launches (tools/stamps.py, persist_phases.py),
                           13 neither stores nor loads, and does not carry, the per-UE state on the inner TTIs of a launch (what "lean_state" can
                           save at most; wrong results, timing only) */
#endif
#ifndef RANENV_KEEP_STATE
#define RANENV_KEEP_STATE 1     /* the multi-TTI builds of one env per wave or more hand the rest of a UE's state to the next warm TTI in registers
                                   (step_body's KEEPS); 0: they only skip the stores nobody reads, like the packed-waves build (A/B builds) */
#endif

namespace ranenv_dev {

enum { MODE_STEP = 0, MODE_DENSE = 1, MODE_RESET = 2,
       MODE_PE = 4 };   // ORed into a step / dense build's MODE: RANENV_F_SCALE_PER_ELEMENT (the masked SE sum scales every element by BW / R before adding)

// ---------------------------------------------------------------------------------------------
// kernel parameters
// ---------------------------------------------------------------------------------------------
// The handle's arrays are few allocations ("slabs") with many equally shaped fields each (field k of a slab at
// k * stride): one base pointer per slab in the kernel arguments instead of one per field.  50 pointers cost 100
// SGPRs, more than a wave has; the step kernel kept spilling them to VGPR lanes and reading them back.
struct Tables {  // scenario pool on the device, rows of [n_scenarios]
    int32_t *slice_i32;  // [NS][S][8] active, has_req, nues, buffer_size, buffer_latency, message_size, nparams, sorted
    double  *slice_f64;  // [NS][S][2] priority, traffic
    int32_t *param_i32;  // [NS][S][3][2] metric, op -- in the slice's own order (the head kernel), then the same BY METRIC (the step kernel):
                         // [NS][S][3][2] declared?, op of metric m (a later parameter for the same metric has overwritten an earlier one)
    double  *param_f64;  // [NS][S][3] value in the slice's own order, then [NS][S][3] value of metric m (1.0 where undeclared)
    int32_t *slice_ues;  // [NS][S][Us]
    int32_t *slot;       // [3][NS][S*16] slot_ue (UE id, -1 = empty slot), slot_mp, slot_pk (its max_pkts / pkt_size)
    int32_t *slice_usecase;                 // [NS][S] SchedColORAN: bit 0 eMBB, bit 1 URLLC
    int32_t *ue;         // [2][6][NS][U] ue_slice, ue_pos, ue_pkt_size, ue_max_pkts, ue_max_age, lane_ue -- all in LANE order: lane l
                         // of the step kernel owns UE lane_ue[l].  Set 0 (compact steps): a scenario's UEs in slices first
                         // (ascending UE id), the idle ones behind them, so that the waves beyond the last UE in a slice have
                         // nothing to step.  Set 1 (full-width launches): lane l = UE l, the coalesced order for the SE stream
};

struct State {
    int32_t *u4;         // [11][B][U] 4-byte per-UE fields (the ST_* accessors below name them)
    int64_t *u8;         // [4][B][U]  8-byte per-UE fields: queue_age_sum, win_sent, win_dropped (int64), se_mean (double)
    int32_t *b4;         // [9][B]     per-env counters
    int2 *age_ring; int32_t *ring_sent; int32_t *ring_drop;
    int8_t *mask_inter, *mask_intra; double *policy_scores;
};
enum { N_U4 = 11, N_U8 = 4, N_B4 = 9, N_TUE = 12 };
#define ST_queue_pkts(p) ((p).st.u4 + (size_t)(0) * (size_t)(p).BU)
#define ST_front(p) ((p).st.u4 + (size_t)(1) * (size_t)(p).BU)
#define ST_front_rem(p) ((p).st.u4 + (size_t)(2) * (size_t)(p).BU)
#define ST_fifo(p) ((p).st.u4 + (size_t)(3) * (size_t)(p).BU)
#define ST_pkt_incoming(p) ((p).st.u4 + (size_t)(4) * (size_t)(p).BU)
#define ST_pkt_throughputs(p) ((p).st.u4 + (size_t)(5) * (size_t)(p).BU)
#define ST_pkt_effective_thr(p) ((p).st.u4 + (size_t)(6) * (size_t)(p).BU)
#define ST_dropped_pkts(p) ((p).st.u4 + (size_t)(7) * (size_t)(p).BU)
#define ST_rb_start(p) ((p).st.u4 + (size_t)(8) * (size_t)(p).BU)
#define ST_rb_count(p) ((p).st.u4 + (size_t)(9) * (size_t)(p).BU)
#define ST_last_push(p) ((p).st.u4 + (size_t)(10) * (size_t)(p).BU)
#define ST_queue_age_sum(p) ((int64_t *)((p).st.u8 + (size_t)(0) * (size_t)(p).BU))
#define ST_win_sent(p) ((int64_t *)((p).st.u8 + (size_t)(1) * (size_t)(p).BU))
#define ST_win_dropped(p) ((int64_t *)((p).st.u8 + (size_t)(2) * (size_t)(p).BU))
#define ST_se_mean(p) ((double *)((p).st.u8 + (size_t)(3) * (size_t)(p).BU))
#define ST_hist_len(p) ((p).st.b4 + (size_t)(0) * (size_t)(p).B)
#define ST_n_push(p) ((p).st.b4 + (size_t)(1) * (size_t)(p).B)
#define ST_step_no(p) ((p).st.b4 + (size_t)(2) * (size_t)(p).B)
#define ST_se_pos(p) ((p).st.b4 + (size_t)(3) * (size_t)(p).B)
#define ST_trf_pos(p) ((p).st.b4 + (size_t)(4) * (size_t)(p).B)
#define ST_episode_no(p) ((p).st.b4 + (size_t)(5) * (size_t)(p).B)
#define ST_reset_count(p) ((p).st.b4 + (size_t)(6) * (size_t)(p).B)
#define ST_push_total(p) ((p).st.b4 + (size_t)(7) * (size_t)(p).B)
#define ST_clear_mark(p) ((p).st.b4 + (size_t)(8) * (size_t)(p).B)
#define ST_age_ring(p) ((p).st.age_ring)
#define ST_ring_sent(p) ((p).st.ring_sent)
#define ST_ring_drop(p) ((p).st.ring_drop)
#define ST_mask_inter(p) ((p).st.mask_inter)
#define ST_mask_intra(p) ((p).st.mask_intra)
#define ST_policy_scores(p) ((p).st.policy_scores)
#define TB_ue_slice(p) ((p).tab.ue + (size_t)(0) * (size_t)(p).NSU)
#define TB_ue_pos(p) ((p).tab.ue + (size_t)(1) * (size_t)(p).NSU)
#define TB_ue_pkt_size(p) ((p).tab.ue + (size_t)(2) * (size_t)(p).NSU)
#define TB_ue_max_pkts(p) ((p).tab.ue + (size_t)(3) * (size_t)(p).NSU)
#define TB_ue_max_age(p) ((p).tab.ue + (size_t)(4) * (size_t)(p).NSU)
#define TB_lane_ue(p) ((p).tab.ue + (size_t)(5) * (size_t)(p).NSU)
#define TB_slot_ue(p) ((p).tab.slot + (size_t)(0) * (size_t)(p).NSL)
#define TB_slot_mp(p) ((p).tab.slot + (size_t)(1) * (size_t)(p).NSL)
#define TB_slot_pk(p) ((p).tab.slot + (size_t)(2) * (size_t)(p).NSL)
#define TB_slice_i32(p) ((p).tab.slice_i32)
#define TB_slice_f64(p) ((p).tab.slice_f64)
#define TB_param_i32(p) ((p).tab.param_i32)
#define TB_param_f64(p) ((p).tab.param_f64)
#define TB_slice_ues(p) ((p).tab.slice_ues)
#define TB_slice_usecase(p) ((p).tab.slice_usecase)

// Work queue of the persistent rollout, one set per workgroup class (hot words on lines of their own).
struct PersistCtl {
    unsigned fresh[8][32];            // [x][0]: cursor into shard x of the class's env list (entries x, x + 8, x + 16, ...)
    int spare; int pad0[31];
    unsigned exited; unsigned pad5[31];   // workgroups of this launch that have left: the last one resets the cursors for the next launch
    int abort; int pad1[31];          // a wait gave up: every workgroup leaves
    struct { unsigned head; unsigned pad2[31]; unsigned tail; unsigned pad3[31]; int avail; int pad4[31]; } q[8];   // ready queue of XCD x: head / tail tickets (monotonic), entries committed and not yet claimed
    unsigned long long stat[8][16];   // per XCD (a line each): [0] chunks kept, [1] pushes, [2] pops, [3] fresh takes, [4] polls that found nothing
};

struct KP {
    int B, S, U, R, G, Us, D, L, max_steps, flags, policy, fixed_intra;
    long long BU, NSU, NSL;   // slab strides: B*U, n_scenarios*U, n_scenarios*S*16
    int T;    // R / G: allocation units of the inter-slice split (an integer division costs a wave ~60 instructions: made once, on the host)
    int e0;   // first env of this launch
    int n_tti;       // TTIs this launch steps every env through (>= 1; more than one only inside ranenv_rollout)
    int compact;     // step only the UEs that are in a slice (lanes are ordered slice members first): waves without one leave
                     // at once.  Set by the host when it is exact: UEs outside every slice get no traffic (see idle_traffic_ok)
    double bw_hz, bw_per_rb, over, norm_traffic, norm_ues, norm_se;
    Tables tab;
    State st;
    const ranenv_episode *episodes;
    const float *se_pool; long long se_stride;   // RB-major or RB-quad-major pool (streaming kernels); the UE-major copy for the gather kernels
    int se_quad;                                 // the bound pool is RB-quad-major [R/4][U][4] (ranenv_bind_se_pool_quad); explicit per-step tiles stay RB-major
    const double *se_mean_pool;                  // gather kernels: [tile][U] mean SE over the RBs of every pooled tile (sidecar)
    int se_rp;                                   // gather kernels: floats per UE row of the UE-major copy (R rounded up to 8)
    // launches of several TTIs (option "lean_state"): != 0 = only an env's last TTI before it can go cold -- the launch's last, a persistent
    // chunk's last -- stores the per-UE state that the next TTI of the same workgroup has in registers, and that TTI does not load it back
    // (step_body's FLUSH / KEEPS); 0 = every TTI stores and loads all of it.  Sits in what was padding behind se_rp: no other member moved
    int lean_state;
    const int32_t *trf_pool;
    // counter-based traffic (ranenv_set_traffic_generator): Poisson draws keyed (seed; env id, episode, step, UE)
    int trf_gen; int env_id_base; unsigned long long trf_seed;
    const unsigned long long *pois_cdf;   // [NS][S][256] floor(P(X <= k) * 2^64), saturated
    const uint8_t *pois_guide;            // [NS][S][64]  smallest k with cdf[k] > j * 2^58
    const int32_t *max_steps_env;         // [B] per-env episode length or null (= max_steps)
    double *acc;                          // [B][8] running sums of the current episode (ranenv_enable_metrics) or null
    // per-call inputs (may be null)
    const uint8_t *env_mask;
    const double *scores; const uint8_t *intra; const double *traffic_bits; const float *se_tiles;
    const uint8_t *dense;
    // outputs (may be null)
    float *obs_inter; float *obs_intra; double *reward; uint8_t *done;
    // alternative heads (SchedTWC / SchedColORAN), bound by ranenv_bind_head_outputs
    float *head_obs; double *head_reward;
    // persistent rollout (ranenv_persist_kernel): this launch's workgroup class
    const int32_t *p_list;            // the class's envs
    int p_count, p_chunk;             // how many; TTIs of an env between two visits of the work queue
    const int32_t *m_list;            // mixed step launches (ranenv_core_kernel_mixed): the narrow class's envs (p_list: the wide class's)
    const int32_t *m_counts;          // ... and how many there are of each, on the device ([0] narrow, [1] wide): no host read-back
    struct PersistCtl *p_ctl;         // the class's counters and per-XCD queue heads
    unsigned long long *p_slots;      // [8][p_cap] queue entries {index + 1, item}
    int p_cap;                        // entries per queue (a power of two >= the batch)
    // launches of several TTIs (option "lean_tail"): != 0 = only an env's last TTI of the launch runs the whole observation tail and
    // stores the outputs nobody can read in between (step_body's LEAN); 0 = every TTI does.  Sits in what was padding in front of
    // p_err: no other member moved
    int lean_tail;
    int *p_err;                       // sticky error word of the handle (a wait gave up), in host memory mapped for the device
    // member lines (ranenv_core_kernel_members / ranenv_persist_kernel_members): the handle's per-UE line copy of the bound pool,
    // floats between two tiles' copies (U x lines per UE x 32); null: the variant is off
    const float *ml_pool; long long ml_stride;
};
static_assert(offsetof(KP, p_err) - offsetof(KP, lean_tail) == 4 && offsetof(KP, lean_tail) - offsetof(KP, p_cap) == 4, "KP: lean_tail fills the padding behind p_cap");
static_assert(offsetof(KP, trf_pool) - offsetof(KP, lean_state) == 4 && offsetof(KP, lean_state) - offsetof(KP, se_rp) == 4, "KP: lean_state fills the padding behind se_rp");

constexpr int WAVE = 64;
constexpr int GRP = 16;   // lanes per (env) group in alloc1/obs and per (env, slice) group in alloc2

struct AdvanceArgs {
    const uint8_t *done; uint8_t *mask;
    ranenv_episode *episodes; const ranenv_episode *table; int table_first, table_n;
    int32_t *episode_no, *reset_count;
    int initial, max_ep, random, env_id_base; unsigned long long seed;
    const float *obs_inter, *obs_intra, *head_obs; float *term_inter, *term_intra, *term_head;
    int n_inter, n_intra, n_head;
    int e0;                                       // first env of this launch (batch partitions)
    int *cls_flag;                                // set when an env restarts: the class lists of the mixed / persistent launches are stale
    const double *acc; double *ep_acc; int32_t *ep_n; int ep_slots;   // episode metrics: running sums -> per-episode log
    const double *head_acc; double *head_ep_acc;                      // ... and the head rewards' pair [B][2] -> [B][ep_slots][2] (null: none)
    const double *slice_acc; double *slice_ep_acc; int32_t *slice_ep_scenario; int n_slice;   // ... and the per-slice sums [B][n_slice = S * 10] -> [B][ep_slots][n_slice], with the finished episode's scenario row [B][ep_slots] (null: none)
};

// Policy network (ranenv_policy.hip): one MLP as packed in the handle's buffer.  Every width is padded with zeros to a multiple of
// 32 (padded rows of W and entries of b are 0, so padded activations are act(0) = 0 and padded inputs add nothing).
enum { NET_MAX_LAYERS = 5, NET_MAX_WIDTH = 512, NET_ROWS = 32 };   // NET_ROWS: GEMM rows (envs / env x slice) per workgroup
struct PolicyNet {
    const float *w;                       // packed [layer]: W [np][kp] row-major, then b [np].  prec RANENV_NET_BF16: W is bf16 (RNE of
                                          // the caller's f32, half the floats), b stays f32; w_off / b_off count floats either way
    long long w_off[NET_MAX_LAYERS], b_off[NET_MAX_LAYERS];
    int kp[NET_MAX_LAYERS], np[NET_MAX_LAYERS];
    int n_layers;                         // Linear layers: hidden ones + the output layer
    int act;                              // RANENV_ACT_*
    int layout;                           // RANENV_NET_IN_*
    int in_dim, out_dim;                  // unpadded
    int prec;                             // RANENV_NET_F32 / RANENV_NET_BF16 (include/ranenv.h: the numeric contract of a bf16 net); sits in
                                          // what was padding in front of slice_stride: no other member moved
    long long slice_stride;               // sliced intra launches (non-shared intra policies): floats between two consecutive slices' packed
                                          // copies, slice s's at w + s * slice_stride; 0 = one net for all slices.  Read by no other kernel
};
// One launch's inputs and action outputs.  A head policy's launch (RANENV_POLICY_HEAD_NETWORK: one row per env, scores into the same
// buffer) has the bound head observation [B][10*S] as its obs_inter and reads no masks.
static_assert(sizeof(PolicyNet) == 160, "PolicyNet: prec fills the padding in front of slice_stride");
struct PolicyIO {
    int B, S, Us, W;                      // W = 2 * Us + 9
    int dist;                             // head: RANENV_HEAD_DIST_*
    int stochastic, env_id_base;
    unsigned long long seed;
    const float *obs_inter, *obs_intra;
    const float *log_std;                 // head, GAUSS_CLIP: [S] the policy's state-independent parameter (null for GAUSS_TANH)
    const int8_t *mask_inter, *mask_intra;
    const int32_t *episode_no, *step_no;
    double *scores; uint8_t *intra;
};
// ranenv_collect / ranenv_collect_head: what the policy launch of one TTI records, every pointer already at that TTI's slot of the
// caller's trajectory (null = not recorded), and the critics it runs behind the actors for the same rows.  A head record: obs_inter =
// its obs_head, action_inter = its action, cols = 1.
struct PolicyRec {
    float *obs_inter, *obs_intra; int8_t *mask_inter, *mask_intra;
    double *action_inter; uint8_t *action_intra;
    float *logp, *vf;                     // [B][cols] of the slot: column 0 by the inter / head launch, column s + 1 by the intra launch
    int cols;                             // S + 1, head: 1
    int intra_actor, intra_critic;        // 0: the inter launch writes zeros into columns 1..S of logp / vf
    int critic_only;                      // the pass behind the last TTI: no actors, no record, vf of the observation as it stands
    int split;                            // host side only: bit 0 / 1 = the inter (head) / intra critic runs as a launch of its own behind the actor's
};
// A population (ranenv_set_population): member m owns envs [first[m], first[m + 1]) and its own copy of every population net.  By value
// in the arguments of the population kernels: a launch carries the grouping it was enqueued under.
enum { POP_MAX = 64 };
struct PopMap { int n; int first[POP_MAX + 1]; };
// THE POPULATION GEOMETRY, one function for the kernel, launch_kind's grid and ranenv_population_tiles: member m's share of a launch
// over envs [e0, e0 + n_envs) with rows_per_env rows per env (kind 0: 1, the flat intra rows: S) -- `rows` rows (0: none) from row
// `row0` of the launch on, in the tiles (workgroups of NET_ROWS rows) the function returns.  Workgroups are numbered member-major.
struct PopShare { int row0, rows; };
__host__ __device__ inline int pop_member_tiles(const int *first, int m, int e0, int n_envs, int rows_per_env, PopShare &sh)
{
    const int lo = first[m] > e0 ? first[m] : e0, hi = first[m + 1] < e0 + n_envs ? first[m + 1] : e0 + n_envs;
    sh.row0 = (lo - e0) * rows_per_env;
    sh.rows = hi > lo ? (hi - lo) * rows_per_env : 0;
    return (sh.rows + NET_ROWS - 1) / NET_ROWS;
}
// The nets of one TTI's policy launches.  head: `actor` / `critic` are the head policy's (one launch, no intra nets), else the inter
// pair.  Null: intra = no intra actor (then vintra is null too), critic / vintra = no critic of that kind.
// pop non-null: a population acts -- net X has a copy per member at X->w + m * stride[X] (floats; in the order actor, intra, critic,
// vintra; 0: one net for every member), and a kind with such a net takes the population kernels.
// tab[X] non-null for the nets of a kind (ranenv_set_population_policy_mixed / _value_mixed: a role of that kind is bound with members
// of differing shape): the kind takes the mixed kernels, which read member m's descriptor of net X from the device table tab[X]
// (POP_MAX entries; entry m's .w is member m's packed copy; a net the launch does not run: tab_none, a table of zeros -- n_layers 0) in place of
// "X's layout + m * stride[X]"; lds[X]: the largest policy_lds_bytes over the table's entries.
struct PolicyNets {
    bool head; const PolicyNet *actor, *intra, *critic, *vintra; const PopMap *pop = nullptr; long long stride[4] = {0, 0, 0, 0};
    const PolicyNet *tab[4] = {nullptr, nullptr, nullptr, nullptr}, *tab_none = nullptr; size_t lds[4] = {0, 0, 0, 0};
};
// THE policy launch entry, for envs [e0, e0 + n_envs).  rec null: the acting launches (actors only; the critics are not read).  rec
// non-null: the recording launches -- actor + critic per agent kind fused, or split by rec's bits; critic_only: the critics alone.  An
// intra launch whose actor or critic has a slice_stride takes the sliced kernels (one workgroup column per slice).
hipError_t launch_policy(hipStream_t, const PolicyNets &, const PolicyIO &, const PolicyRec *rec, int e0, int n_envs);
size_t policy_lds_bytes(const PolicyNet &);
// ranenv_sac_targets: one call's rows and outputs (include/ranenv.h spells out the arithmetic).  The actor is a GAUSS_TANH head net,
// q1 / q2 two nets of one shape on [next_obs | action].
struct SacArgs {
    long long n; int S;
    const float *next_obs, *reward; const uint8_t *done;      // [n][10*S], [n], [n]
    double gamma, ent_coef;
    int stochastic; unsigned long long seed, draw;
    float *target, *next_action, *next_logp, *q;              // [n]; [n][S], [n], [n][2] or null
};
hipError_t launch_sac_targets(hipStream_t, const PolicyNet &actor, const PolicyNet &q1, const PolicyNet &q2, const SacArgs &);

// ranenv_ppo_update (ranenv_ppo.hip; include/ranenv.h "PPO update"): one net of the update -- its layout (net.w unused), the slot's packed
// weights, Adam moments and gradient scratch (member m's at + m * stride floats, `floats` of them in use; n_layers 0: not bound / not updated)
struct PpoNet { PolicyNet net; float *w, *m, *v, *g; long long stride, floats; };
// ... and one call: actor and critic per kind (0 inter, 1 intra), the members' shares of the row lists, the record
struct PpoArgs {
    PpoNet net[2][2];                     // [kind][0 the actor, 1 the critic]
    int first[2][POP_MAX + 1];            // kind k, member m: entries [first[k][m], first[k][m + 1]) of every epoch's list
    const int32_t *order[2]; long long order_stride[2];      // [max_epochs][order_stride[k]] record rows
    int T, B, S, Us, W;
    const ranenv_ppo_hparams *hp;         // device, [members]
    ranenv_trajectory traj;
    int32_t *t;                           // [POP_MAX][2] Adam step counters
    int max_epochs;
    double *stats;                        // [members][2][max_epochs][RANENV_PPO_STATS]
    float *grad; long long grad_stride;   // [members][2][grad_stride] or null
    float *probe_logp;                    // [T][B][S + 1] or null (ranenv_ppo_probe_logp)
};
// Bytes of LDS the update of this actor / critic pair needs (critic null or n_layers 0: none); the rule is in include/ranenv.h
size_t ppo_lds_bytes(const PolicyNet &actor, const PolicyNet *critic);
enum { PPO_LDS_MAX = 160 * 1024 };
// A mixed population's update (ranenv_ppo_bind_mixed), beside PpoArgs: workgroup (m, kind) takes net k's shape from entry m of tab[kind][k]
// -- the role's device table the mixed policy kernels read, or the table of zeros for a role that is not bound -- and its packed floats
// from floats[role * POP_MAX + m] (device, written at bind and re-bind; 0: not bound).  PpoNet's net / floats are member 0's there:
// read for "is the role bound" alone.  lds: the largest ppo_lds_bytes over the members and the kinds of the call.
struct PpoMixed { const PolicyNet *tab[2][2]; const long long *floats; };
// A wide binding's update (ranenv_ppo_bind_wide), beside PpoArgs: two row buffers in LDS, and workgroup (m, kind) parks every layer's 32
// input rows in its own `stride` floats of `scratch` at (m * 2 + kind) * stride -- slab l at stride net_ld(kp[l]), back to back; actor and
// critic run one after the other and share it.  The LDS bytes and scratch floats of one actor / critic pair under that plan:
struct PpoWide { float *scratch; long long stride; };
size_t ppo_wide_lds_bytes(const PolicyNet &actor, const PolicyNet *critic);
long long ppo_wide_scratch(const PolicyNet &actor, const PolicyNet *critic);
// mixed null: the uniform instance; wide non-null: the wide instance of either
hipError_t launch_ppo_update(hipStream_t, int n_members, size_t lds, const PpoArgs &, const PpoMixed *mixed, const PpoWide *wide = nullptr);
// ranenv_ppo_update_slices (ranenv_ppo_bind_slices): 1 + n_slices workgroups -- workgroup 0 the inter pair (net[0], first[0][0..1], hp[0]),
// workgroup 1 + s slice s's intra pair: net[1]'s copies at s * stride, entries [first[1][s], first[1][s + 1]) of the intra lists.  t, stats,
// grad and the wide scratch are numbered by workgroup: [1 + S] in place of [members][2].  n_slices 0: the inter pair alone.
hipError_t launch_ppo_update_slices(hipStream_t, int n_slices, size_t lds, const PpoArgs &, const PpoWide *wide);
// ranenv_ppo_update under ranenv_ppo_bind_spread (ranenv_ppo_spread.hip; include/ranenv.h "One agent over the chip"): ONE agent's update,
// three launches per optimiser step.  THE GEOMETRY of one kind's schedule, one function for the host (launch grids,
// ranenv_ppo_spread_plan) and the three kernels: n rows in minibatches of `minibatch` entries, `epochs` times -- optimiser step `step`
// is minibatch step % per_epoch of epoch step / per_epoch, entries [c0, c0 + nb) of the epoch's list, in `tiles` tiles of NET_ROWS rows
// that `grid` = min(tiles, slabs) workgroups walk: workgroup w the tiles w, w + grid, ... into gradient slab w.
enum { PPO_SPREAD_BLOCK = 1024,           // floats of a kind's packed gradient (actor, then critic) per block of the reduce and the apply
       PPO_SPREAD_STATS = 6,              // doubles per slab: policy loss, entropy, logp_old - logp, clipped, live rows, value loss
       PPO_SPREAD_SLABS_MAX = 256 };
struct PpoSpreadStep { int ep, mb, c0, nb, tiles, grid; };
__host__ __device__ inline int ppo_spread_per_epoch(int n, int minibatch) { return n > 0 ? (int)(((long long)n + minibatch - 1) / minibatch) : 0; }
__host__ __device__ inline PpoSpreadStep ppo_spread_step(int n, int minibatch, int slabs, int step)
{
    PpoSpreadStep g;
    const int per_epoch = ppo_spread_per_epoch(n, minibatch);
    g.ep = step / per_epoch; g.mb = step - g.ep * per_epoch;
    g.c0 = g.mb * minibatch; g.nb = n - g.c0 < minibatch ? n - g.c0 : minibatch;
    g.tiles = (g.nb + NET_ROWS - 1) / NET_ROWS; g.grid = g.tiles < slabs ? g.tiles : slabs;
    return g;
}
// One kind's share of the binding's buffers and of the call: every array is written by one launch and read by later ones alone
struct PpoSpreadKind {
    float *slab; long long slab_stride;   // [slabs][slab_stride]: the actor's packed gradient, then the critic's; zero between two steps
    float *park; long long park_stride;   // wide: [slabs][park_stride] parked rows
    double *bpart;                        // [blocks] the reduce blocks' sums of squares
    double *wstat;                        // [slabs][PPO_SPREAD_STATS] the pass workgroups' row statistics
    double *run;                          // [RANENV_PPO_STATS] the epoch's running sums between two steps (PpoEpoch's fields in order)
    int32_t *t0;                          // the kind's step counter as the call found it (the first pass copies it)
    int n, steps, blocks;                 // rows of an epoch's list, optimiser steps of the call (0: the kind is not updated), reduce / apply blocks
};
struct PpoSpreadArgs {
    PpoArgs a;                            // nets, lists, record, counters t[kind], stats [2][max_epochs][RANENV_PPO_STATS], grad [2][grad_stride]; a.hp unused
    ranenv_ppo_hparams hp;
    PpoSpreadKind k[2];
    int slabs, step;
};
// The three launches of optimiser step a.step (grid_pass / blocks: the larger kind's); wide: the pass under the wide plan
hipError_t launch_ppo_spread_step(hipStream_t, size_t lds, const PpoSpreadArgs &, bool wide);
// ranenv_ppo_update_slices under ranenv_ppo_bind_slices_spread (include/ranenv.h "Nets per slice over the chip"): the per-slice
// binding's 1 + S policies under the same three launches, blockIdx.y the UNIT u -- unit 0 the inter pair (kind 0, `mem` 0), unit 1 + s
// slice s's intra pair (kind 1, `mem` s), ppo_update_body<.., SLICES>'s numbering.  `p` is the spread binding's argument block with
// p.a as ranenv_ppo_update_slices fills it (first[1][s]: the slices' shares; t, stats and grad numbered by unit) and p.k[kind] the
// buffers of the kind's FIRST unit: all slices have one shape, so unit 1 + s's lie at p.k[1]'s pointers + s x the strides below, and
// no table per unit goes into the arguments.  p.k[kind].steps is 0 or 1 there -- is the kind trained by this call? -- and .n unused:
// a unit's rows n_u = first[kind][mem + 1] - first[kind][mem] and steps = epochs x ppo_spread_per_epoch(n_u, minibatch) are computed
// where they are needed, on the device and for the launch grids, by ppo_slices_spread_unit.
struct PpoSpreadSlices {
    long long slab_unit, park_unit;       // floats between two slices' slabs ([slabs][slab_stride]) and parked rows ([slabs][park_stride])
    long long dbl_unit;                   // doubles between two units' block partials, slab statistics and running sums
    int n_units;                          // 1 + S, or 1: the inter pair alone
};
struct PpoSpreadSlicesArgs { PpoSpreadArgs p; PpoSpreadSlices x; };
// THE UNIT GEOMETRY, one function for the kernels, the launch grids and ranenv_ppo_slices_spread_plan: unit u's kind and `mem`, the
// first entry `lo` and the count `n` of its share of every epoch's list, and its optimiser steps (saturated at 2^31 - 1, which the
// host refuses before any launch)
struct PpoSliceUnit { int kind, mem, lo, n, steps; };
__host__ __device__ inline PpoSliceUnit ppo_slices_spread_unit(const int (*first)[POP_MAX + 1], int u, int epochs, int minibatch)
{
    PpoSliceUnit x;
    x.kind = u > 0 ? 1 : 0; x.mem = u > 0 ? u - 1 : 0;
    x.lo = first[x.kind][x.mem]; x.n = first[x.kind][x.mem + 1] - x.lo;
    const long long steps = (long long)epochs * ppo_spread_per_epoch(x.n, minibatch);
    x.steps = steps > 0x7fffffffLL ? 0x7fffffff : (int)steps;
    return x;
}
// The three launches of optimiser step a.p.step: the pass grid (the largest grid of that step over the live units, n_units), the
// elementwise grid (the larger kind's blocks, n_units); units and blocks beyond their own extent return
hipError_t launch_ppo_spread_slices_step(hipStream_t, size_t lds, const PpoSpreadSlicesArgs &, bool wide);
// ... under ranenv_ppo_bind_spread_bfloat (include/ranenv.h "bf16 nets over the chip"): the nets are RANENV_NET_BF16 ones.  PpoNet of such a
// net: `net` the ACTING copy's layout (bf16 W, two per float); w the f32 MASTER copy Adam steps, and m, v, g, `floats`, all in the F32
// packed layout, the slabs' and dev_grad's.  Beside it that layout's offsets, the acting copy the pass's forward reads
// (acting == bf16(master) behind every apply) and the transposed bf16 copy its backward product reads: layer l's Wt [kp][np] at float
// net.w_off[l] of `wt`.
struct PpoBf16Net { long long w_off[NET_MAX_LAYERS], b_off[NET_MAX_LAYERS]; float *acting, *wt; };
struct PpoSpreadBf16Args { PpoSpreadArgs p; PpoBf16Net bf[2][2]; };      // bf[kind][0 the actor, 1 the critic]
// Bytes of LDS of a bf16 pair's pass: PPO_FIXED and the larger net's rows -- bf16 rows of the input and every hidden layer at stride
// net_ld16, the output layer's f32 rows
size_t ppo_bf16_lds_bytes(const PolicyNet &actor, const PolicyNet *critic);
hipError_t launch_ppo_spread_step_bf16(hipStream_t, size_t lds, const PpoSpreadBf16Args &);
// master and wt of one net from its acting copy (the bind and every re-bind): bf16 W widened, f32 biases copied, Wt transposed
hipError_t launch_ppo_bf16_seed(hipStream_t, const PolicyNet &net, const PpoBf16Net &bf, float *master, long long floats);

// ranenv_ppo_update_head (include/ranenv.h "PPO update of the head policies"): the head actor and critic (net[0], net[1]; stride unused),
// the handle's log_std [S] with its moments and gradient scratch, the call's hyper-parameters by value, the row lists
// [max_epochs][n_rows] and the ranenv_collect_head record.  One workgroup.
struct PpoHeadArgs {
    PpoNet net[2];
    float *log_std, *ls_m, *ls_v, *ls_g;  // [S] each
    const int32_t *order; int n_rows;
    int T, B, S;
    ranenv_ppo_hparams hp;
    ranenv_head_trajectory traj;
    int32_t *t;                           // the one Adam step counter
    double *stats;                        // [max_epochs][RANENV_PPO_STATS]
    float *grad;                          // [actor floats + critic floats + S] or null
};
hipError_t launch_ppo_update_head(hipStream_t, size_t lds, const PpoHeadArgs &);
// ranenv_ppo_update_head under ranenv_ppo_bind_head_spread (ranenv_ppo_spread.hip; include/ranenv.h "Head policies over the chip"): the
// head binding's own buffers -- never the IBSched spread binding's -- and optimiser step `step` of `steps`; the geometry is
// ppo_spread_step(a.n_rows, a.hp.minibatch, slabs, step).  Every array is written by one launch and read by later ones alone.
struct PpoHeadSpread {
    float *slab; long long slab_stride;   // [slabs][slab_stride]: the actor's packed gradient, then the critic's; zero between two steps
    double *gls;                          // [slabs][S] the pass workgroups' d/d log_std, unrounded
    double *bpart;                        // [blocks] the reduce blocks' sums of squares (block 0's with log_std's)
    double *wstat;                        // [slabs][PPO_SPREAD_STATS] the pass workgroups' row statistics
    double *run;                          // [RANENV_PPO_STATS] the epoch's running sums between two steps
    int32_t *t0;                          // the step counter as the call found it (the first pass copies it)
    int slabs, step, steps, blocks;
};
struct PpoHeadSpreadArgs { PpoHeadArgs a; PpoHeadSpread k; };
// The three launches of optimiser step a.k.step
hipError_t launch_ppo_spread_head_step(hipStream_t, size_t lds, const PpoHeadSpreadArgs &);

// ranenv_ppo_row_count / ranenv_ppo_row_order (ranenv_rows.hip; include/ranenv.h "Row lists on the device").  THE GEOMETRY of the
// compaction, by value in the kernels' arguments: the record's T x B x S cells are cut into chunks of at most ROWS_CHUNK cells that lie
// in ONE unit each, numbered unit-major -- unit u's are chunk_first[u] .. chunk_first[u + 1] - 1, in ascending order of their cells.
// Grouping MEMBERS: unit m is the member of envs [first_env[m], first_env[m + 1]); at one TTI its cells are contiguous in [t][b][s] and
// take chunks_per[m] chunks, TTI-major.  Grouping SLICES: unit s is slice s, its cells the record rows t * B + b at that s, ROWS_CHUNK
// rows per chunk (first_env = {0, B}: the inter kind's one unit).
enum { ROWS_CHUNK = 2048 };
struct RowsGeom { int T, B, S, grouping, units, n_chunks; int chunk_first[POP_MAX + 1], chunks_per[POP_MAX], first_env[POP_MAX + 1]; };
// One kind's lists: out[k][p] for epochs k0 <= k < k0 + (the launch's epochs) and 0 <= p < n = first[units], the kind's table;
// first_env: the inter kind's env ranges (one per unit); base: the intra kind's compacted cells
struct RowsShuffle {
    int kind, units, B, k0; long long n; unsigned long long seed;
    int first[POP_MAX + 1], first_env[POP_MAX + 1];
    const int32_t *base; int32_t *out;
};
// (enqueue only; errors through hipGetLastError)  count + scan: counts / offsets [n_chunks], first [units + 1]
void launch_rows_count(hipStream_t, const RowsGeom &, const int8_t *mask, int32_t *counts, int32_t *offsets, int32_t *first);
void launch_rows_compact(hipStream_t, const RowsGeom &, const int8_t *mask, const int32_t *offsets, int32_t *base, long long n_base);
void launch_rows_shuffle(hipStream_t, int epochs, const RowsShuffle &);

// ranenv_sac_update (ranenv_sac.hip; include/ranenv.h "SAC update"): one gradient step is a critic pass, an apply, an actor pass and
// a second apply.  A net of a pass: its layout (net.w unused) and the packed weights the pass reads.
struct SacNet { PolicyNet net; const float *w; };
// One pass over one minibatch of n rows: workgroup w of `grid` walks tiles w, w + grid, ... and adds into gradient slab w -- tensor x
// (0 actor, 1 q1, 2 q2) at slab + w * slab_stride + off[x] -- and writes its share of the statistics into partial[w][8] (the critic
// pass entries 0..4, the actor pass 5..7).  first_row: the global index of the minibatch's row 0, the rows' Philox counter.
struct SacPassArgs {
    SacNet actor, q[2], qt[2];            // the head actor, the live critics, the target critics
    float *slab; long long slab_stride, off[3];
    double *partial;
    long long n, first_row; int S;
    const float *obs, *action, *reward, *next_obs; const uint8_t *done;      // the minibatch's rows
    double gamma, target_entropy; unsigned long long seed, draw;
    const float *log_ent_coef;            // the coefficient's logarithm as the previous step left it
    float *target;                        // [n] or null
};
// The elementwise launch behind a pass: segment k (workgroup row k) sums its `floats` elements of the `used` slabs in ascending order,
// zeroes them, and steps Adam at counter t (SAC_OP_ADAM: w, m, v; grad non-null: the gradient is stored there), and / or moves
// tgt towards w (SAC_OP_POLYAK).  last != 0, the step's second apply: thread 0 of workgroup (0, 0) sums the partials, steps the
// coefficient ent = {log_ent_coef, m, v} (auto_coef) at counter t_ent, writes the step's eight statistics and the counters.
enum { SAC_OP_ADAM = 1, SAC_OP_POLYAK = 2 };
struct SacApplySeg { float *w, *m, *v, *tgt, *grad; long long slab_off, floats; int t, op; };
struct SacApplyArgs {
    SacApplySeg seg[3]; int n_seg;
    float *slab; long long slab_stride; int used;
    double lr, tau;
    int last, auto_coef, t_ent; long long n;
    float *ent; const double *partial; double *stats; float *grad_ent;
    int32_t *dev_t; int32_t t_new[4];
};
// Bytes of LDS of the passes for this actor / critic shape: the fixed region and the larger net's 32 rows of all layers
size_t sac_lds_bytes(const PolicyNet &actor, const PolicyNet &critic);
hipError_t launch_sac_pass(hipStream_t, int which, int grid, size_t lds, const SacPassArgs &);      // which: 0 the critic pass, 1 the actor pass
hipError_t launch_sac_apply(hipStream_t, const SacApplyArgs &);

enum { PERSIST_ENV_BITS = 20 };          // persistent rollout: queue item = env | TTIs done << 20
constexpr int CORE_NT = GRP * GRP;   // 256 = largest U = threads of the widest step-kernel block

// ---------------------------------------------------------------------------------------------
// Launch table
// ---------------------------------------------------------------------------------------------
// Builds of the step kernel (all from step_body, ranenv_step_body.hpp)
enum StepBuild {
    SB_LEAN = 0,        // ranenv_core_kernel<MODE, NP, MANY>: batches that fill the chip (5 waves per SIMD)
    SB_SMALL,           // ranenv_core_kernel_small: <= 8 workgroups per CU (4 waves per SIMD, deeper SE queue)
    SB_GATHER,          // ranenv_core_kernel_gather: SE gather mode
    SB_TINY1,           // ranenv_core_kernel_tiny1: one-TTI step launches of a batch at <= 2 waves per SIMD (whole row in flight)
    SB_MIXED,           // ranenv_core_kernel_mixed<NP, MANY, GATHER>: one block per wide env + one per two narrow envs
    SB_PACKED,          // ranenv_core_kernel_packed<8, MANY, GATHER>: two envs per wave (NP = 8 only)
    SB_PERSIST,         // ranenv_persist_kernel<GATHER, NP>: work-queue rollout
    SB_PERSIST_TINY,    // ranenv_persist_kernel_tiny<NP>: the same at <= 2 waves per SIMD, streaming only
};
struct StepLaunch {
    int np;             // row width of the build: 8, 10, 16
    int build;          // StepBuild
    int mode;           // MODE_STEP / MODE_DENSE / MODE_RESET, | MODE_PE for the per-element builds (lean / gather only)
    bool many;          // a launch of several TTIs (MODE_STEP only)
    bool gather;        // SB_MIXED / SB_PACKED / SB_PERSIST: the SE gather build
    bool members = false;   // SB_LEAN (step, several TTIs, not per-element) / SB_PERSIST (streaming): the build that reads the member-lines copy
};
// ranenv_step.hip, one object per row width.  hipErrorInvalidDeviceFunction: that combination is not built.
// ev0 / ev1 non-null: an extended launch that records the dispatch's own start / stop timestamps.
hipError_t launch_step_np8(const StepLaunch &, dim3 grid, dim3 block, hipStream_t, hipEvent_t ev0, hipEvent_t ev1, const KP &);
hipError_t launch_step_np10(const StepLaunch &, dim3 grid, dim3 block, hipStream_t, hipEvent_t ev0, hipEvent_t ev1, const KP &);
hipError_t launch_step_np16(const StepLaunch &, dim3 grid, dim3 block, hipStream_t, hipEvent_t ev0, hipEvent_t ev1, const KP &);
const void *step_kernel_ptr_np8(const StepLaunch &);      // (for occupancy / attribute queries)
const void *step_kernel_ptr_np10(const StepLaunch &);
const void *step_kernel_ptr_np16(const StepLaunch &);
size_t shared_core_bytes_np8();
size_t shared_core_bytes_np10();
size_t shared_core_bytes_np16();
inline hipError_t launch_step(const StepLaunch &l, dim3 grid, dim3 block, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1, const KP &kp)
{
    switch (l.np) {
    case 8: return launch_step_np8(l, grid, block, s, ev0, ev1, kp);
    case 10: return launch_step_np10(l, grid, block, s, ev0, ev1, kp);
    default: return launch_step_np16(l, grid, block, s, ev0, ev1, kp);
    }
}
inline const void *step_kernel_ptr(const StepLaunch &l)
{
    return l.np == 8 ? step_kernel_ptr_np8(l) : (l.np == 10 ? step_kernel_ptr_np10(l) : step_kernel_ptr_np16(l));
}
inline size_t shared_core_bytes(int np) { return np == 8 ? shared_core_bytes_np8() : (np == 10 ? shared_core_bytes_np10() : shared_core_bytes_np16()); }

// ranenv_aux.hip: the small kernels (enqueue only; errors through hipGetLastError)
void launch_classify(hipStream_t, const ranenv_episode *eps, const int32_t *members, int B, int n_class, int one_class, int32_t *list,
                     int32_t *count, int *flag, int force);
void launch_se_sidecar(hipStream_t, unsigned n_tiles, unsigned block, const float *pool, long long stride, long long tile0, int U, int R, int Rp,
                       int quad, double *mean, float *um);
void launch_se_sidecar_from_power(hipStream_t, unsigned n_tiles, unsigned block, const double *power, long long tile0, int U, int R, int Rp,
                                  double tx, double noise, double *mean, float *um);
void launch_se_retile_quad(hipStream_t, unsigned blocks, const float *src, float *dst, long long n_quads, int U, int R);
// Member-lines copy (ranenv_numeric.hpp, "Member lines") of tiles [0, n_tiles) of an RB-major (quad 0) or RB-quad-major pool: dst
// [n_tiles][U][lines][32].  The plan's lines by value: first RB, whole 8-RB groups held (0: the tail line, which holds `tail` RBs)
enum { MEMBER_LINES_MAX = 24 };
struct MemberLineTable { int lines, tail; int rb0[MEMBER_LINES_MAX], groups[MEMBER_LINES_MAX]; };
void launch_se_retile_member_lines(hipStream_t, unsigned blocks, const float *src, long long src_stride, int quad, float *dst, long long n_tiles,
                                   int U, int R, const MemberLineTable &, long long packed_f4 = 0);
// the packed copy (ranenv_se_retile_member_lines_packed): packed_f4 = float4s per tile of the output (the tile stride), see ranenv_member_lines_packed_layout
// ranenv_build_se_stats: stats [n][4][U] (mean, std, min, max per UE over the R RBs) of tiles [tile0, tile0 + n_tiles), the sidecar launch's shape
void launch_se_tile_stats(hipStream_t, unsigned n_tiles, unsigned block, const float *pool, long long stride, long long tile0, int U, int R,
                          int quad, double *stats);
// ranenv_rbs_needed: n_episodes * n_steps workgroups of `block` >= U threads write the per-step rows, then one workgroup per episode
// its mean row (n_episodes * n_steps < 2^31: the host checks)
struct RbsArgs {
    const ranenv_episode *eps; int n_steps;
    const double *stats;                  // [tiles][4][U]
    const int32_t *ue_slice;              // [NS][U], entry u = UE u
    const int32_t *slice_i32; const double *slice_f64;      // Tables' rows
    int S, U, R; double bw_mhz;
    double *slice_out;                    // [n_ep][T][S][RANENV_LOAD_SLICE_COLS] or null
    double *net_out;                      // [n_ep][T][3]
};
void launch_rbs_needed(hipStream_t, unsigned n_episodes, unsigned block, const RbsArgs &, double *episode_mean);
void launch_se_from_power(hipStream_t, unsigned blocks, const double *power, float *se, long long n, double tx_per_rb, double noise);
void launch_ddiv_selftest(hipStream_t, const double *a, const double *b, double *fast, double *ieee, long long n);
// head_acc: the per-env running pair of the two head rewards [B][2] or null; reset != 0: the launch follows a reset (the pair of the
// envs under the mask is zeroed), else a step (this TTI's rewards are added)
void launch_head(hipStream_t, dim3 grid, dim3 block, const KP &, double *head_acc, int reset);
// Per-slice episode sums [B][S][RANENV_SLICE_METRIC_COLS] behind a step (reset == 0: this TTI's share is added; reads kp.reward and kp.obs_intra)
// or behind a reset (reset != 0: the rows of the envs under kp.env_mask are zeroed); block = the head kernel's
void launch_slice_metrics(hipStream_t, dim3 grid, dim3 block, const KP &, double *slice_acc, int reset);
// Device traces (ranenv_bind_trace): one row of every recorded env of a step launch's range.  `env` / `slot`: the recorded envs in
// ascending order and the column each owns; the launch covers entries [first, first + n) of them, one workgroup each.  The pool is
// the bound float32 one (RB-major or RB-quad-major) whatever the SE mode -- never the gather kernels' UE-major copy that KP carries
// there.  Reads the step's outputs through kp (collect's redirected reward / done slots included).
struct TraceArgs {
    const int32_t *env, *slot; int first;
    int32_t *count, *lost;
    const float *se_pool; long long se_stride; int se_quad;
    ranenv_trace out;                     // (out.envs is the caller's host array: not read on the device)
};
void launch_trace(hipStream_t, unsigned n, const KP &, const TraceArgs &);
void launch_advance(hipStream_t, unsigned n_envs, const AdvanceArgs &);
// reward_stride: doubles between two (env, column) entries' rewards' rows, i.e. reward[(t * B + b) * reward_stride + c] (n_cols: packed)
void launch_gae(hipStream_t, int n_steps, int B, int n_cols, const double *reward, int reward_stride, const float *vf, const uint8_t *done,
                double gamma, double lambda, float *adv, float *vtarg);
// ... with a (gamma, lambda) pair per population member (ranenv_set_population_gae / ranenv_gae_population): env b's lanes take the pair
// of the member that owns b.  By value in the kernel's arguments, like the grouping.
struct GaePop { PopMap pop; double gamma[POP_MAX], lambda[POP_MAX]; };
void launch_gae_pop(hipStream_t, int n_steps, int B, int n_cols, const double *reward, int reward_stride, const float *vf, const uint8_t *done,
                    const GaePop &, float *adv, float *vtarg);
// Entries [m0, m0 + n) of a population role's descriptor table: `proto` with .w advanced by `stride` floats per entry
void launch_net_table(hipStream_t, PolicyNet *tab, int m0, int n, const PolicyNet &proto, long long stride);
void launch_idle_traffic(hipStream_t, unsigned n_eps, const ranenv_episode *eps, const int32_t *pool, int U, const int32_t *lane_slice,
                         const int32_t *lane_ue, int *violations);
// ranenv_collect_replay: up to two ranges of 8-byte words copied device to device in one launch (n1 = 0: one range)
void launch_copy_words(hipStream_t, unsigned long long *dst0, const unsigned long long *src0, long long n0, unsigned long long *dst1,
                       const unsigned long long *src1, long long n1);
// ranenv_replay_sample: n rows gathered from the ring's first n_rows = min(written, C) * B transitions
struct ReplaySampleArgs {
    long long n, n_rows; int B, S, reward_col;
    int reward_cols;                      // doubles per ring reward row: 2 (the head kernel's pair) or S + 1 (the step's row, RANENV_HEAD_SRC_INTER)
    unsigned long long seed, draw;
    const float *ring_obs, *ring_next_obs; const double *ring_action, *ring_reward; const uint8_t *ring_done;
    float *obs, *action, *reward, *next_obs; uint8_t *done; long long *index;
};
void launch_replay_sample(hipStream_t, const ReplaySampleArgs &);
// A bf16 net's layer: the caller's f32 W [N][K] -> bf16 [np][kp] at dst (round to nearest even), zeros in the padding
void launch_pack_bf16(hipStream_t, const float *src, int N, int K, int np, int kp, unsigned short *dst);

}  // namespace ranenv_dev
