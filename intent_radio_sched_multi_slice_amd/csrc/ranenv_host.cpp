// ranenv_host.cpp -- host side of the C ABI in include/ranenv.h: handles, validation, pools, launch schedules (partitions, rollouts,
// persistent work-queue launches, ranges), options, episode advance.  Plain C++ on the HIP runtime API; every kernel is reached through
// the launch table of ranenv_internal.h.
#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <new>
#include <string>
#include <array>
#include <vector>

#include "ranenv_internal.h"

using namespace ranenv_dev;

namespace {
thread_local std::string g_last_error;
constexpr int N_STEP_BUILDS = SB_PERSIST_TINY + 1;          // (StepBuild, ranenv_internal.h)

}  // namespace

// What a net is for (the first four: the ABI's role numbers of the IBSched nets), and the forms an IBSched role is bound in, in rising
// precedence (ranenv::serving)
enum NetRole { NET_INTER, NET_INTRA, NET_INTER_VALUE, NET_INTRA_VALUE, NET_HEAD_CLIP, NET_HEAD_TANH, NET_HEAD_VALUE, NET_SAC_Q };
enum NetForm { FORM_ONE, FORM_SLICE, FORM_MEMBER };

struct ranenv {
    ranenv_config cfg;
    KP kp;
    std::vector<void *> allocs;
    std::string err;
    int nt = 0;                                 // threads of the core kernel (one per UE, whole waves)
    int nslot = 0;                              // threads of the head kernel (one per slot, whole waves)
    int n_cus = 256;                            // compute units of the device (ranenv_create)
    // pools
    bool have_scenarios = false;
    int64_t se_tiles_n = 0, trf_rows_n = 0;   // extents of the bound pools (0 = none)
    unsigned long long *d_pois_cdf = nullptr; uint8_t *d_pois_guide = nullptr;
    std::vector<double> slice_traffic;          // [NS][S] host copy (traffic generator tables)
    std::vector<int32_t> slice_has_req;
    std::vector<int32_t> members_host; int32_t *d_members = nullptr;      // [NS] UEs in slices per scenario
    // SE gather mode (ranenv_set_se_mode): sidecars of the bound pool, owned by the handle
    int se_mode = RANENV_SE_STREAM;
    double *d_se_mean = nullptr; float *d_se_um = nullptr; int se_rp = 0;
    // member lines (option "member_lines"): the handle's packed per-UE line copy of the bound pool, per tile [U][nlw][32] + tail block [U][8], that compact
    // streaming rollouts read instead of whole tiles (ml_stride floats per tile).  Built by the first rollout that would use it;
    // a rebind of the pool invalidates it (the buffer stays for the rebuild); ml_failed: the allocation failed, the variant is off
    float *d_ml = nullptr; int64_t ml_cap = 0; long long ml_stride = 0; bool ml_valid = false, ml_failed = false;
    int member_lines = -1;         // -1 auto / 0 off / 1 on
    int last_rollout_member_lines = 0;          // the last ranenv_rollout call's step launches read the copy (read-only option)
    // scenario load (ranenv_build_se_stats / ranenv_rbs_needed): per-tile statistics of the bound pool [se_stats_n][4][U] (se_stats_n = 0: none
    // valid; the buffer of se_stats_cap tiles stays for the next build), and the call's staging: descriptors, network rows
    double *d_se_stats = nullptr; int64_t se_stats_n = 0, se_stats_cap = 0;
    ranenv_episode *d_load_eps = nullptr; int64_t load_eps_cap = 0;
    double *d_load_net = nullptr; int64_t load_net_cap = 0;
    // compact steps (KP::compact): allowed while UEs outside every slice provably receive no traffic
    bool idle_check_dirty = true, pool_idle_zero = false, table_idle_zero = false;
    bool idle_state_clean = true;               // no step so far can have given an idle UE packets (else: full width until a full reset)
    int *d_violations = nullptr;
    // episodes and auto-reset
    ranenv_episode *d_episodes = nullptr;
    bool have_episodes = false;
    ranenv_episode *d_ep_table = nullptr; int ep_table_first = 0, ep_table_n = 0;     // auto-reset: episode number -> descriptor
    int ar_initial = 0, ar_max = 0, ar_random = 0; unsigned long long ar_seed = 0; bool ar_on = false;
    uint8_t *d_ar_mask = nullptr;
    int32_t *d_max_steps = nullptr;
    std::vector<int32_t> host_max_steps;        // copy of ranenv_set_max_steps' array (the multi-episode rollout follows the step counters)
    double *d_acc = nullptr, *d_ep_acc = nullptr; int32_t *d_ep_n = nullptr; int ep_slots = 0;   // ranenv_enable_metrics
    double *d_slice_acc = nullptr, *d_slice_ep_acc = nullptr; int32_t *d_slice_ep_scn = nullptr;    // ranenv_enable_slice_metrics: [B][S][10], [B][ep_slots][S][10], [B][ep_slots]
    bool slice_on = false;                      // ... switched on (the slice-metrics kernel follows every step and reset; off with kp.acc)
    // ranenv_bind_trace: the caller's ring, the recorded envs in ascending order with the column each owns (host copies and, in one
    // device array of 4 * trace_cap words: envs, columns, count, lost), an outgrown array staying allocated until ranenv_destroy
    ranenv_trace trace{}; bool trace_on = false;
    std::vector<int32_t> trace_env, trace_slot;
    int32_t *d_trace = nullptr; int trace_cap = 0;
    // Host shadow of the per-env step counters (what they will be once everything enqueued so far has run): `done` is a function of
    // the counter alone (step >= the env's episode length), so ranenv_autoreset knows WITHOUT reading anything back whether an episode
    // ended at the TTI just enqueued -- and enqueues nothing when none did (an RL loop calls it behind every step: three small launches
    // = 7 us per TTI saved, profiles/r05_ab_log.txt).  Valid from a reset of the whole batch until something the host cannot follow
    // (a masked reset by the caller).
    std::vector<int32_t> sh_steps; bool sh_valid = false;
    const uint8_t *last_done = nullptr;         // the `done` buffer the steps write (the shortcut applies to that buffer only)
    // persistent launches, and the class lists they share with mixed blocks
    int32_t *d_plist = nullptr, *d_pcount = nullptr; PersistCtl *d_pctl = nullptr; unsigned long long *d_pslots = nullptr;
    int p_nclass = 0, p_cap = 0;
    std::vector<int32_t> pcount_host; bool pclass_dirty = true, pcount_host_stale = true;
    bool pclass_maybe = false;     // an auto-reset ran since the lists were built: they are stale IF an env restarted (the device knows:
    int *d_cls_flag = nullptr;     // ... this word, set by ranenv_advance_kernel, tested and cleared by the classify kernel)
    int *h_perr = nullptr;         // sticky error word of the persistent launches, in host memory the device can write (a wait gave up)
    int *d_perr_dev = nullptr;     // ... its address as the device sees it
    int perr_seen = 0;             // ... what of it has been reported
    int last_rollout_persistent = 0, last_rollout_launches = 0;   // what the last ranenv_rollout call ran (read-only options)
    long long last_rollout_kept_state_ttis = 0;   // ... and the TTIs they enqueued without the per-UE state's stores (option "lean_state": n_tti - 1 per launch)
    long long last_rollout_lean_ttis = 0;   // ... and the TTIs its step launches enqueued without the observation tail (option "lean_tail": n_tti - 1 per launch)
    // MODE_STEP launches of the step kernel that succeeded since ranenv_create, per StepBuild; [1]: those of several TTIs (read-only options
    // "step_launches_<build>" / "..._many").  Enqueues: a replayed graph counts once, at its capture.
    uint64_t step_launches[N_STEP_BUILDS][2] = {};
    std::string launch_note;       // a failed step launch: which build had no kernel (appended to the call's error message by fail())
    int p_wave_slots[2] = {0, 0};  // wave slots per CU of the persistent kernel (streaming, gather build), from the occupancy query
    // batch partitions (ranenv_set_partitions): envs [part_lo[k], part_lo[k+1]) are stepped by their own launch on
    // their own stream, so that one partition's ramp and tail run under the other partitions' steady state
    int n_parts = 1;
    std::vector<hipStream_t> part_stream;
    std::vector<hipEvent_t> part_done, part_in;
    std::vector<int> part_lo;
    hipEvent_t ev_in = nullptr;
    // ranenv_profile_begin / _end: the dispatch's own start / stop timestamps of every step-kernel launch
    // (hipExtLaunchKernel's events: valid with further launches queued behind, unlike events recorded between launches)
    bool prof_on = false;
    std::vector<hipEvent_t> prof_ev;            // pairs (start, stop), one per launch
    size_t prof_used = 0;
    long long prof_ttis = 0;       // TTIs covered by the launches timed since ranenv_profile_begin
    long long prof_env_ttis = 0;   // env-TTIs covered by the launches timed since ranenv_profile_begin
    // One bound net set: its copies' packed weights in a buffer of the slot's own (cap floats; an outgrown buffer stays allocated until
    // ranenv_destroy, and a slot keeps its buffers while off).  member[i]: copy i's descriptor as the device sees it (.w = its address),
    // member_dims[i]: its unpadded widths -- one entry for one net, one (slice 0's, the S copies standing at its slice_stride) for nets
    // per slice, G entries at member_stride for a population's.  `mixed` (ranenv_set_population_policy_mixed / _value_mixed): the members
    // may differ in shape; member_stride, the extent of every member, is the largest member's packed size.
    struct NetSlot {
        int role; NetForm form;          // the IBSched role (-1: a head or SAC net) and the form of it: set once, here
        NetSlot(int role_ = -1, NetForm form_ = FORM_ONE) : role(role_), form(form_) {}
        PolicyNet net{}; bool on = false; float *w = nullptr; long long cap = 0; long long member_stride = 0;
        bool mixed = false; std::vector<PolicyNet> member; std::vector<std::array<int32_t, 6>> member_dims; size_t lds_max = 0;
        float *opt = nullptr; long long opt_cap = 0;      // ranenv_ppo_bind: Adam's m, v and the gradient scratch, opt_cap floats each, in the packed layout
        // net -- copy 0's descriptor, PolicyNets points at it -- and lds_max, the largest copy's LDS need, follow from member[]
        void derive() { net = member[0]; lds_max = 0; for (const PolicyNet &x : member) lds_max = std::max(lds_max, policy_lds_bytes(x)); }
    };
    // THE ROLE TABLE: the IBSched nets by the ABI's role number (NetRole: 0 inter actor, 1 intra actor, 2 inter critic, 3 intra critic)
    // and form -- one net (ranenv_set_policy_network / _value_network), one per slice (ranenv_set_intra_policy_networks / _intra_value_networks:
    // roles 1 and 3), one per member (ranenv_set_population_policy / _value).  Which forms a binding call switches on and off: BIND_RULES.
    NetSlot nets[4][3] = {{{0, FORM_ONE}, {0, FORM_SLICE}, {0, FORM_MEMBER}}, {{1, FORM_ONE}, {1, FORM_SLICE}, {1, FORM_MEMBER}},
                          {{2, FORM_ONE}, {2, FORM_SLICE}, {2, FORM_MEMBER}}, {{3, FORM_ONE}, {3, FORM_SLICE}, {3, FORM_MEMBER}}};
    // ranenv_set_head_policy_network / _head_value_network: SchedTWC / SchedColORAN's actor and critic on the head observation;
    // ranenv_set_sac_critics.  One form each.
    NetSlot head, head_value, sac_q1, sac_q2;
    PopMap pop{};      // ranenv_set_population: the grouping (pop.n = 0: none)
    // The population roles' descriptor tables on the device: [5][POP_MAX] entries in the order actor, intra, critic, vintra, then a table
    // of zeros (n_layers 0: no net).  Allocated by the first population bind and never moved; every population bind writes its role's
    // table on the caller's stream, and a one-net slot that serves a role beside a mixed one gets G entries of its one net.
    PolicyNet *d_pop_tab = nullptr;
    // THE PRECEDENCE RULE: the slot that serves role r now -- the population's nets if on, else the nets per slice if on, else the one
    // net if on, else null (no net of that role acts)
    NetSlot *serving(int r) { for (int f = FORM_MEMBER; f >= FORM_ONE; f--) if (nets[r][f].on) return &nets[r][f]; return nullptr; }
    const NetSlot *serving(int r) const { return const_cast<ranenv *>(this)->serving(r); }
    const PolicyNet *serving_net(int r) const { const NetSlot *s = serving(r); return s ? &s->net : nullptr; }
    // ... and the slot role r's device table describes while a mixed role is bound: nets per slice have no entries there
    const NetSlot *tabled(int r) const { return nets[r][FORM_MEMBER].on ? &nets[r][FORM_MEMBER] : (nets[r][FORM_ONE].on ? &nets[r][FORM_ONE] : nullptr); }
    bool pop_bound() const { for (int r = 0; r < 4; r++) if (nets[r][FORM_MEMBER].on) return true; return false; }
    bool pop_mixed() const { for (int r = 0; r < 4; r++) if (nets[r][FORM_MEMBER].on && nets[r][FORM_MEMBER].mixed) return true; return false; }
    // THE PPO BINDING of the IBSched nets: what ranenv_ppo_bind (plain), _bind_mixed (mixed: a mixed population, each member on its own
    // shape), _bind_wide (wide: the wide plan, with or without mixed), _bind_slices (slices: one intra pair per slice, with or without
    // wide) or _bind_spread (slabs > 0: ONE agent, every optimiser step spread over up to `slabs` workgroups per kind, with or without
    // wide; slices and slabs > 0: _bind_slices_spread, the per-slice units under the spread schedule) bound, and the geometry that
    // follows from it, stated here alone.  A handle has one; a binding that ends is `{}` again, so no flag outlives `on`.  An update
    // UNIT is what one optimiser trains: member m's pair of a kind, or (slices) the inter pair and slice s's intra pair; a spread
    // binding has the one member's two.
    struct PpoBinding {
        bool on = false, mixed = false, wide = false, slices = false;
        int slabs = 0;                                                                                        // > 0: the spread binding
        bool bf16 = false;                                                                                    // ... of RANENV_NET_BF16 nets (ranenv_ppo_bind_spread_bfloat)
        int units(int kind, int members, int S) const { return slices ? (kind == 1 ? S : 1) : members; }      // ... of a kind
        int workgroups(int members, int S) const { return slabs ? 2 * slabs : (slices ? 1 + S : 2 * members); }      // ... of an update launch at most
        // unit u of `kind` by workgroup number: its step counter in d_ppo_t and (not spread) its share of the parked rows in d_ppo_park
        int wg(int kind, int u) const { return slices ? (kind ? 1 + u : 0) : u * 2 + kind; }
        // the entry point the messages name (parked: where they speak of the parked rows, which ranenv_ppo_bind_wide allocates)
        const char *entry(bool parked = false) const { return bf16 ? "ranenv_ppo_bind_spread_bfloat" : slabs ? (slices ? "ranenv_ppo_bind_slices_spread" : "ranenv_ppo_bind_spread") : (slices ? "ranenv_ppo_bind_slices" : (parked ? "ranenv_ppo_bind_wide" : "ranenv_ppo_bind")); }
    } ppo;
    // ... its step counters by workgroup number [POP_MAX * 2], the call's hyper-parameters on the device [POP_MAX], the diagnostic
    // log-probability buffer the NEXT update takes and forgets
    int32_t *d_ppo_t = nullptr; ranenv_ppo_hparams *d_ppo_hp = nullptr; float *ppo_probe = nullptr;
    // mixed: the packed floats of member m's net of role r on the device, [4][POP_MAX] (0: the role is not bound), written at that
    // bind and at every re-bind under it
    long long *d_ppo_floats = nullptr, ppo_floats[4][POP_MAX] = {};      // (... and the host copy the upload reads)
    // wide: the parked rows of the workgroups, [workgroups][ppo_park_stride] floats, allocated at that bind (an outgrown one stays
    // allocated, like the weights'), never by an update
    float *d_ppo_park = nullptr; long long ppo_park_stride = 0, ppo_park_cap = 0;
    // spread: the gradient slabs [2][slabs][the kind's actor + critic floats] (zero between two optimiser steps), and per kind the reduce
    // blocks' sums of squares [ppo_spread_blocks], the pass workgroups' statistics [PPO_SPREAD_SLABS_MAX][PPO_SPREAD_STATS] and the
    // epoch's running sums [RANENV_PPO_STATS] in one array of doubles; the parked rows (wide) lie in d_ppo_park, [2][slabs][the kind's
    // need].  The call's copy of the two step counters: d_ppo_t[2], [3] (a spread binding has one member: [0], [1] are its counters).
    // All allocated at the bind, never by an update.  ranenv_ppo_bind_slices_spread: the same arrays per UNIT (unit 0 the inter pair,
    // unit 1 + s slice s) -- the slabs and parked rows of unit 0, then the slices' back to back; the doubles [ppo_spread_units] times
    // one kind's; the call's copies of the 1 + S counters at d_ppo_t[POP_MAX + u]
    float *d_ppo_slab = nullptr; long long ppo_slab_cap = 0;
    double *d_ppo_spread = nullptr; long long ppo_spread_blocks = 0; int ppo_spread_units = 0;
    // ranenv_ppo_bind_spread_bfloat: per role the trained bf16 net's f32 state in the F32 packed layout -- master, m, v, g, ppo_bf_cap[r]
    // floats each -- and behind them the transposed bf16 copy, ppo_bf_cap16[r] floats (the acting copy's packed size).  Allocated at the
    // bind (an outgrown one stays allocated), seeded from the acting copy at the bind and at every re-bind of the role
    float *d_ppo_bf[4] = {nullptr, nullptr, nullptr, nullptr}; long long ppo_bf_cap[4] = {0, 0, 0, 0}, ppo_bf_cap16[4] = {0, 0, 0, 0};
    // ranenv_ppo_bind_head / ranenv_ppo_update_head: bound?, the one step counter, and log_std's Adam moments and gradient scratch
    // [3][S] (m, v, g); the actor's and the critic's lie on the head and head_value slots (opt)
    bool ppo_head_on = false; int32_t *d_ppo_head_t = nullptr; float *d_head_ls_opt = nullptr;
    // ranenv_ppo_bind_head_spread: the head binding's form (slabs > 0: every optimiser step spread over up to `slabs` workgroups) and
    // its own buffers, none shared with the IBSched spread binding's: the gradient slabs [slabs][actor + critic floats] (zero between two
    // optimiser steps), and in one array of doubles gls [slabs][S], the reduce blocks' sums of squares [ppo_head_blocks], the pass
    // workgroups' statistics [PPO_SPREAD_SLABS_MAX][PPO_SPREAD_STATS] and the epoch's running sums [RANENV_PPO_STATS].  The call's
    // copy of the step counter: d_ppo_head_t[1].  All allocated at the bind, never by an update
    int ppo_head_slabs = 0;
    float *d_ppo_head_slab = nullptr; long long ppo_head_slab_cap = 0;
    double *d_ppo_head_spread = nullptr; long long ppo_head_blocks = 0; int ppo_head_gls_slabs = 0;
    // ranenv_sac_bind / ranenv_sac_update: bound?, the packed floats of the actor and of one critic at the bind (a re-bind of another
    // size ends the binding), the slab count, the coefficient's mode and the target entropy; the live critics with their moments
    // [6][sac_q_cap] (q1, q2, m of both, v of both), the actor's moments [2][sac_a_cap], the gradient slabs [slabs][actor + 2 critics],
    // the passes' partial sums [256][8], the coefficient {log_ent_coef, m, v, -} and the tensors' step counters [4] (actor, q1, q2,
    // coefficient) with their host shadow: every launch is enqueued in order, so the host knows the counters without reading them
    bool sac_on = false; long long sac_af = 0, sac_qf = 0; int sac_slabs = 0, sac_auto = 0; double sac_target_entropy = 0.0;
    float *d_sac_q = nullptr; long long sac_q_cap = 0;
    float *d_sac_a_opt = nullptr; long long sac_a_cap = 0;
    float *d_sac_slab = nullptr; long long sac_slab_cap = 0;
    double *d_sac_partial = nullptr; float *d_sac_ent = nullptr; int32_t *d_sac_t = nullptr; int32_t sac_t[4] = {0, 0, 0, 0};
    // ranenv_ppo_row_count / ranenv_ppo_row_order: the last count's arguments, geometry and host tables (valid: a count succeeded and
    // ranenv_ppo_row_order may follow it), the chunks' counts and offsets [2][chunks_cap] with the units' table [POP_MAX + 1] behind
    // them in one array, and the compacted cells [base_cap].  The arrays grow with the record (the outgrown one is freed) and are
    // the handle's own until ranenv_destroy
    struct RowLists {
        bool valid = false; int n_steps = 0, grouping = 0; const int8_t *mask = nullptr; PopMap pop{};
        RowsGeom geom{}; int first[2][POP_MAX + 1] = {};
        int32_t *d_chunks = nullptr; long long chunks_cap = 0;
        int32_t *d_base = nullptr; long long base_cap = 0;
    } rows;
    // ranenv_set_population_gae: a (gamma, lambda) pair per member for ranenv_collect's GAE pass
    bool gae_on = false; double gae_gamma[POP_MAX] = {}, gae_lambda[POP_MAX] = {};
    // The IBSched nets of a TTI's launches as they are bound (critics: a recording's), with the population map where a member's copy acts
    PolicyNets ibsched_nets(bool critics) const
    {
        PolicyNets n{false, serving_net(NET_INTER), serving_net(NET_INTRA), critics ? serving_net(NET_INTER_VALUE) : nullptr,
                     critics ? serving_net(NET_INTRA_VALUE) : nullptr};
        if (pop_bound()) {
            n.pop = &pop;
            // a kind with a mixed-bound role (of the nets this launch may run) reads every net of it through the tables
            bool mx[2] = {false, false};
            for (int r = 0; r < 4; r++) {
                const NetSlot &p = nets[r][FORM_MEMBER];
                n.stride[r] = p.on ? p.member_stride : 0;
                if (p.on && p.mixed && (critics || r < NET_INTER_VALUE)) mx[r & 1] = true;
            }
            n.tab_none = d_pop_tab + 4 * POP_MAX;
            for (int r = 0; r < 4; r++) {
                if (!mx[r & 1]) continue;
                n.tab[r] = d_pop_tab + r * POP_MAX;
                n.lds[r] = tabled(r) ? tabled(r)->lds_max : 0;
            }
        }
        return n;
    }
    // ... and the actions the step reads under RANENV_POLICY_NETWORK / _HEAD_NETWORK (shared: one policy acts at a time)
    int net_stochastic = 0; unsigned long long net_seed = 0;
    double *d_net_scores = nullptr; uint8_t *d_net_intra = nullptr;
    int head_dist = 0, head_stochastic = 0; unsigned long long head_seed = 0;
    int head_src = RANENV_HEAD_SRC_HEAD;        // ranenv_set_head_policy_source: where the head nets' rows and the recorded rewards come from
    float *d_head_log_std = nullptr;
    double *d_head_acc = nullptr, *d_head_ep_acc = nullptr;      // episode sums of the two head rewards [B][2], their log [B][ep_slots][2]
    // off-policy collection (ranenv_bind_replay): the caller's ring and how many TTIs it has taken
    ranenv_replay ring{}; bool ring_on = false; long long ring_written = 0;
    int collect_split = -1;        // option "collect_split": the critic of ranenv_collect in a launch of its own (1), fused behind the actor (0), -1 = by weight size
    // options (the table `options` below, include/ranenv.h "Options")
    bool compact_enabled = true;                // option "compact"
    int fuse = 0;                  // TTIs per launch inside ranenv_rollout: 0 = chosen per rollout, n = at most n (1 = off)
    std::vector<int> fuse_first;   // override of the length of partition k's first launch of a rollout (RANENV_FUSE_FIRST=a,b,c)
    int np = 16;                                // row width of the step kernel's build: max(S, Us) rounded up to 8, 10 or 16
    bool small_batch = false;                   // at most 8 workgroups per CU: the 128-VGPR build with the deeper SE queue
    int tiny_step = 1;                          // option "tiny_step": one-TTI step launches of a batch at <= 2 waves per SIMD run the whole-row build
    int persist = -1;              // ranenv_rollout as one persistent work-queue launch per workgroup class (option "persist"):
                                   // 0 never, 1 whenever possible, -1 (default) where it was measured to win: SE gather mode with a
                                   // batch that fills the CUs, and either mode with a batch of <= 2 waves per SIMD
    int persist_chunk = 10;        // TTIs of an env between two visits of the work queue
    int persist_grid = 0;          // experiment: cap on the workgroups of a persistent launch, in wave slots (0 = what the chip holds)
    bool pack = true;              // two envs per wave where the sizes allow (option "pack")
    int mix = 1;                   // whole-batch step launches of two-wave workgroups as mixed blocks (option "mix"): 0 never, 1 where the
                                   // batch does not fit the chip anyway (auto), 2 also for batches that do (tests)
    int persist_inject = 0;        // test hook (option "persist_inject_abort"): the next persistent launch finds its abort word set
    int autoreset_shortcut = 0;                 // option "autoreset_shortcut" (default 0: ranenv_autoreset reads dev_done, every env with a non-zero flag restarts)
};

namespace {

int fail(ranenv_handle h, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    std::string msg = buf;
    if (h && !h->launch_note.empty()) { msg += " [" + h->launch_note + "]"; h->launch_note.clear(); }
    if (h) h->err = msg;
    g_last_error = msg;
    return code;
}

#define HIP_TRY(h, call)                                                                       \
    do {                                                                                       \
        hipError_t e_ = (call);                                                                \
        if (e_ != hipSuccess) return fail(h, RANENV_E_HIP, "%s: %s", #call, hipGetErrorString(e_)); \
    } while (0)

template <typename T>
int dev_alloc(ranenv_handle h, T **out, size_t count)
{
    void *ptr = nullptr;
    size_t bytes = count * sizeof(T);
    if (bytes == 0) bytes = sizeof(T);
    hipError_t e = hipMalloc(&ptr, bytes);
    if (e != hipSuccess) return fail(h, RANENV_E_NOMEM, "hipMalloc(%zu): %s", bytes, hipGetErrorString(e));
    e = hipMemset(ptr, 0, bytes);
    if (e != hipSuccess) return fail(h, RANENV_E_HIP, "hipMemset: %s", hipGetErrorString(e));
    h->allocs.push_back(ptr);
    *out = (T *)ptr;
    return RANENV_OK;
}

size_t NS_all(ranenv_handle h) { return (size_t)h->cfg.n_scenarios * (size_t)h->cfg.n_slices; }

// Inversion tables of the traffic generator, one row per (scenario, slice): cdf[k] = floor(P(X <= k) * 2^64) for
// X ~ Poisson(slice Mbps), k = 0..255 (lower half summed upwards, upper half as 1 - survival, the survival
// function summed from the tail so that the far tail keeps its relative precision), and the 64-entry guide.
int build_poisson_tables(ranenv_handle h, hipStream_t stream)
{
    const size_t rows = NS_all(h);
    if (h->slice_traffic.size() != rows) return RANENV_OK;          // no scenarios yet: built when they are loaded
    std::vector<unsigned long long> cdf(rows * 256, ~0ull);
    std::vector<uint8_t> guide(rows * 64, 0);
    const long double two64 = 18446744073709551616.0L;
    for (size_t r = 0; r < rows; r++) {
        const double lam = h->slice_traffic[r];
        if (!h->slice_has_req[r] || lam == 0.0) continue;          // never sampled
        if (!(lam > 0.0) || lam > 128.0)
            return fail(h, RANENV_E_INVALID, "traffic generator: slice traffic %g Mbps outside (0, 128] (256-entry inversion table)", lam);
        long double pmf[256], ll = logl((long double)lam);
        for (int k = 0; k < 256; k++) pmf[k] = expl((long double)k * ll - (long double)lam - lgammal((long double)k + 1.0L));
        const int mode = (int)lam;
        unsigned long long *c = &cdf[r * 256];
        long double cum = 0.0L;
        for (int k = 0; k <= mode; k++) { cum += pmf[k]; const long double v = floorl(cum * two64); c[k] = v >= two64 ? ~0ull : (unsigned long long)v; }
        long double sf = 0.0L;                                      // P(X > k), from the tail
        for (int k = 255; k > mode; k--) {
            const long double v = ceill(sf * two64);
            c[k] = v <= 0.0L ? ~0ull : (v >= two64 ? 0ull : (unsigned long long)(two64 - v));
            sf += pmf[k];
        }
        c[255] = ~0ull;
        for (int k = 1; k < 256; k++) if (c[k] < c[k - 1]) c[k] = c[k - 1];      // monotone across the seam at the mode
        uint8_t *g = &guide[r * 64];
        int k = 0;
        for (int j = 0; j < 64; j++) {
            const unsigned long long lo = (unsigned long long)j << 58;
            while (k < 255 && c[k] <= lo) k++;
            g[j] = (uint8_t)k;
        }
    }
    if (!h->d_pois_cdf) {
        if (dev_alloc(h, &h->d_pois_cdf, rows * 256) != RANENV_OK || dev_alloc(h, &h->d_pois_guide, rows * 64) != RANENV_OK) return RANENV_E_NOMEM;
    }
    HIP_TRY(h, hipMemcpyAsync(h->d_pois_cdf, cdf.data(), cdf.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, stream));
    HIP_TRY(h, hipMemcpyAsync(h->d_pois_guide, guide.data(), guide.size(), hipMemcpyHostToDevice, stream));
    HIP_TRY(h, hipStreamSynchronize(stream));
    h->kp.pois_cdf = h->d_pois_cdf; h->kp.pois_guide = h->d_pois_guide;
    return RANENV_OK;
}

// RANENV_F_SCALE_PER_ELEMENT: every step / dense launch runs the lean build compiled for that convention -- no mixed blocks, packed
// waves, small-batch / whole-row builds or persistent launches (those exist for the default convention only)
bool scale_per_element(const ranenv *h) { return (h->cfg.flags & RANENV_F_SCALE_PER_ELEMENT) != 0; }

// A batch whose widest blocks all together stay within 2 waves per SIMD (8 per CU): one class, and -- streaming -- the build
// with the whole SE row in flight.
constexpr long long TINY_MAX_WAVES_PER_CU = 8;
bool persist_tiny(const ranenv *h) { return (long long)h->cfg.batch * (h->nt / WAVE) <= TINY_MAX_WAVES_PER_CU * h->n_cus; }

bool stream_capturing(hipStream_t stream)      // (an error of the query itself counts as "capturing": the careful path)
{
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cs) != hipSuccess) { (void)hipGetLastError(); return true; }
    return cs != hipStreamCaptureStatusNone;
}

// Must the handle's other streams wait for `stream`?  Not when it holds nothing: then no signal has to cross between two hardware
// queues.  (hipStreamQuery is illegal on a capturing stream: a caller that graph-captures its step keeps the event.)
bool stream_busy(hipStream_t stream) { return stream_capturing(stream) || hipStreamQuery(stream) != hipSuccess; }

int persist_prepare(ranenv_handle h, hipStream_t stream, bool need_host_counts);

// Packed waves address a per-env row as (uniform array base) + (32-bit row + lane offset), see row_at<2>: every array they
// address that way must stay below 4 GB.  True for every size a packed step makes sense at (the reference's: megabytes); a handle
// with pools beyond that steps one env per wave.
bool pack_fits_32_of(const ranenv_config &cfg, long long trf_rows_n, long long se_tiles_n)
{
    const unsigned long long lim = 1ull << 32, B = (unsigned long long)cfg.batch, U = (unsigned long long)cfg.n_ues,
                             S = (unsigned long long)cfg.n_slices, NS = (unsigned long long)cfg.n_scenarios,
                             D = (unsigned long long)cfg.hist_depth, W = 2ull * cfg.max_ues_slice + 9ull;
    // (one term per array a packed step addresses as base + 32-bit offset, each the array's whole allocation in bytes: the per-UE tables
    // (two lane orders), the per-UE state slabs, the window rings, the slice tables, the intent parameters -- two blocks, the second BY
    // METRIC --, the score rows, the observation rows, the reward rows, the traffic pool / explicit traffic, the gather sidecar of means)
    return (unsigned long long)N_TUE * NS * U * 4 < lim && (unsigned long long)N_U4 * B * U * 4 < lim && (unsigned long long)N_U8 * B * U * 8 < lim &&
           B * D * U * 4 < lim && NS * S * 32 < lim && 2 * NS * S * 24 < lim && NS * S * 16 < lim && B * S * 8 < lim && B * (S + 1) * 8 < lim &&
           B * S * W * 4 < lim && (unsigned long long)trf_rows_n * U * 4 < lim && (unsigned long long)se_tiles_n * U * 8 < lim;
}
bool pack_fits_32(const ranenv *h) { return pack_fits_32_of(h->cfg, h->trf_rows_n, h->se_tiles_n); }

// Under ranenv_profile_begin: the next (start, stop) pair of the event pool, for a launch of n envs through n_tti TTIs
hipError_t prof_events(ranenv_handle h, int n, int n_tti, hipEvent_t *ev0, hipEvent_t *ev1)
{
    *ev0 = nullptr; *ev1 = nullptr;
    if (!h->prof_on) return hipSuccess;
    while (h->prof_ev.size() < h->prof_used + 2) {
        hipEvent_t e = nullptr;
        const hipError_t ce = hipEventCreate(&e);
        if (ce != hipSuccess) return ce;
        h->prof_ev.push_back(e);
    }
    *ev0 = h->prof_ev[h->prof_used]; *ev1 = h->prof_ev[h->prof_used + 1];
    h->prof_used += 2; h->prof_ttis += n_tti; h->prof_env_ttis += (long long)n * n_tti;
    return hipSuccess;
}

// Names of the builds, in StepBuild's order (the read-only options "step_launches_<build>", the message of a failed launch)
const char *const step_build_names[N_STEP_BUILDS] = {"lean", "small", "gather", "tiny1", "mixed", "packed", "persist", "persist_tiny"};

// launch_step with its result kept: a success of a MODE_STEP launch is counted for its build, a failure (no kernel for that build, mode
// and flag combination: a slip of the dispatch) leaves the build's name for the message of the call that fails
hipError_t launch_step_counted(ranenv_handle h, const StepLaunch &l, dim3 grid, dim3 block, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1, const KP &kp)
{
    const hipError_t e = launch_step(l, grid, block, s, ev0, ev1, kp);
    const bool known = l.build >= 0 && l.build < N_STEP_BUILDS;
    if (e == hipSuccess) {
        if (known && (l.mode & 3) == MODE_STEP) h->step_launches[l.build][l.many ? 1 : 0]++;
        if (l.members) h->last_rollout_member_lines = 1;
        // (a build of several TTIs runs the whole observation tail at an env's last TTI of the launch only: KP::lean_tail, step_body's LEAN)
        if ((l.mode & 3) == MODE_STEP && l.many && kp.lean_tail != 0 && kp.n_tti > 1) h->last_rollout_lean_ttis += kp.n_tti - 1;
        // (... and stores the per-UE state at an env's last TTI before it can go cold only: KP::lean_state.  A persistent launch flushes at every
        // chunk end as well: the figure is its upper bound, reached when no chunk ends inside the launch)
        if ((l.mode & 3) == MODE_STEP && l.many && kp.lean_state != 0 && kp.n_tti > 1) h->last_rollout_kept_state_ttis += kp.n_tti - 1;
    } else {
        char buf[160];
        snprintf(buf, sizeof(buf), "step kernel build '%s' (row width %d, mode %d, %s, %s): %s", known ? step_build_names[l.build] : "?", l.np, l.mode,
                 l.many ? "several TTIs" : "one TTI", l.gather ? "gather" : "stream", hipGetErrorString(e));
        h->launch_note = buf;
    }
    return e;
}

// THE STEP BUILD, chosen here and nowhere else, from the handle's shape and options (nothing is written) and what the launch is: mode, TTIs,
// the compact value offered (2: a rollout's), the SE gather build?, envs [e0, e0 + n), a member-lines copy on offer?, an env mask?, the call's own
// SE tiles?  With its grid and block and the compact value (0 / 1) its kernels then read.  SB_MIXED: the class lists are the caller's to sort and bind.
struct StepFacts { int mode, n_tti, compact; bool gather; int e0, n; bool lines = false, masked = false, tiles = false; };
struct StepChoice { StepLaunch l; dim3 grid, block; int compact; };
StepChoice step_choice(const ranenv *h, const StepFacts &f)
{
    const bool step = f.mode == MODE_STEP;
    // RANENV_F_SCALE_PER_ELEMENT: the lean builds with the other rounding of the masked SE sum (MODE_PE); a reset sums no masked row
    const bool pe = f.mode != MODE_RESET && scale_per_element(h);
    const bool many = step && f.n_tti > 1;
    // Compact steps pay off for the gather kernels throughout (-3...-7 %).  The streaming kernels want lane = UE: their row
    // loads are coalesced in that order (a wave reads 256 contiguous bytes per RB; slice members first scatters its lanes
    // over the whole 400-byte row), so they step compactly only where it was measured to win: under ranenv_rollout's
    // overlapping partitions (-4 %; +15 % for two alternating ranges, +1.5 % for one launch per TTI).
    // Mixed blocks (ranenv_core_kernel_mixed): the whole batch in one launch of one block per wide env + one per two narrow envs -- all of it
    // resident in one round.  For launches of the whole batch of two-wave workgroups, where a compact step is exact.
    // (whole-batch launches only: for the ranges of a partitioned batch per-range lists were built and measured -- two alternating
    // ranges 47.8 against 48.0 us per TTI in gather mode, and the streaming kernel loses the lane = UE order it wants there: dropped)
    const bool mixed = step && !pe && h->mix != 0 && f.compact != 0 && h->nt == 2 * WAVE && f.e0 == 0 && f.n == h->cfg.batch && !f.masked &&
                       (h->mix == 2 || !persist_tiny(h)) && (RANENV_DIAG == 0 || RANENV_DIAG == 13);
    const int compact = f.compact != 0 && (mixed || f.gather || f.compact == 2) ? 1 : 0;
    const dim3 grid((unsigned)f.n), block((unsigned)h->nt);
    if (mixed) return {{h->np, SB_MIXED, MODE_STEP, many, f.gather}, grid, dim3(2 * WAVE), compact};      // (grid: an upper bound of wide + ceil(narrow / 2))
    // packed waves: two envs per wave for envs of <= 32 UEs / <= 8 slices (see ranenv_core_kernel_packed)
    if (step && !pe && h->pack && h->np == 8 && h->cfg.n_ues <= 32 && h->nt == WAVE && (f.n & 1) == 0 && !f.masked && pack_fits_32(h))
        return {{8, SB_PACKED, MODE_STEP, many, f.gather}, dim3((unsigned)(f.n / 2)), dim3(WAVE), compact};
    // SE gather mode, else -- one-TTI steps of a batch at <= 2 waves per SIMD -- the whole-row build, else the small-batch or the lean build
    StepLaunch l{h->np, SB_LEAN, pe ? f.mode | MODE_PE : f.mode, many, f.gather};
    if (f.gather) l.build = SB_GATHER;
    else if (!pe && step && !many && h->tiny_step && persist_tiny(h)) l.build = SB_TINY1;
    else if (!pe && h->small_batch) l.build = SB_SMALL;
    // THE MEMBER-LINES RULE, launches per chunk: the lean build of several TTIs reads an offered copy where the step is compact
    l.members = l.build == SB_LEAN && many && !pe && f.lines && compact != 0 && !f.tiles;
    return {l, grid, block, compact};
}
// ... and of a persistent class launch: the work-queue build of the SE mode; streaming, a batch of <= 2 waves per SIMD runs the whole-row
// build, and any other reads an offered member-lines copy.  `plain`: the work-queue build whatever the batch (the occupancy query's).
StepLaunch persist_choice(const ranenv *h, bool lines, bool plain = false)
{
    const bool gather = h->se_mode == RANENV_SE_GATHER, tiny = !gather && !plain && persist_tiny(h);
    return {h->np, tiny ? SB_PERSIST_TINY : SB_PERSIST, MODE_STEP, true, gather, !gather && !tiny && lines};
}
void gather_kp(const ranenv *h, KP &kp)      // the SE gather builds read the sidecars of the bound pool instead of tiles
{
    kp.se_pool = h->d_se_um; kp.se_stride = (long long)h->cfg.n_ues * h->se_rp;
    kp.se_mean_pool = h->d_se_mean; kp.se_rp = h->se_rp;
}

// Per-slice episode metrics are kept: the slice-metrics kernel follows every step and reset, one TTI per step launch
bool slice_metrics_on(const ranenv *h) { return h->slice_on && h->kp.acc != nullptr && h->d_slice_acc != nullptr; }
// ... then a call that steps needs the two outputs that kernel reads
int slice_metrics_outputs(ranenv_handle h, const float *obs_intra, const double *reward)
{
    if (slice_metrics_on(h) && (!obs_intra || !reward))
        return fail(h, RANENV_E_INVALID, "per-slice metrics read the step's dev_reward and dev_obs_intra: both are needed while they are on");
    return RANENV_OK;
}

// A trace is bound: the trace kernel follows every step launch, one TTI per step launch (the conditions slice metrics impose)
bool trace_on(const ranenv *h) { return h->trace_on; }
// ... then a call that steps needs the outputs that kernel copies, and -- for the tile -- a float32 pool or the call's own tiles
int trace_outputs(ranenv_handle h, const float *se_tiles, const float *obs_inter, const float *obs_intra, const double *reward, const uint8_t *done)
{
    if (!trace_on(h)) return RANENV_OK;
    const ranenv_trace &t = h->trace;
    if ((t.obs_inter && !obs_inter) || (t.obs_intra && !obs_intra) || (t.reward && !reward) || (t.done && !done))
        return fail(h, RANENV_E_INVALID, "the bound trace copies the step's dev_obs_inter, dev_obs_intra, dev_reward and dev_done: each one it records is needed while it is bound");
    if (t.se && !se_tiles && !h->kp.se_pool)
        return fail(h, RANENV_E_STATE, "the bound trace records SE tiles: this handle has gather sidecars only (ranenv_bind_se_gather_from_power) and the call gives no explicit tiles");
    return RANENV_OK;
}
// The trace kernel for the recorded envs inside [e0, e0 + n): a range of the ascending list
void launch_trace_range(ranenv_handle h, const KP &kp, int e0, int n, hipStream_t stream)
{
    const auto lo = std::lower_bound(h->trace_env.begin(), h->trace_env.end(), e0), hi = std::lower_bound(lo, h->trace_env.end(), e0 + n);
    if (lo == hi) return;
    TraceArgs a{};
    a.env = h->d_trace; a.slot = h->d_trace + h->trace_cap; a.first = (int)(lo - h->trace_env.begin());
    a.count = h->d_trace + 2 * (size_t)h->trace_cap; a.lost = h->d_trace + 3 * (size_t)h->trace_cap;
    a.se_pool = h->kp.se_pool; a.se_stride = h->kp.se_stride; a.se_quad = h->kp.se_quad;
    a.out = h->trace;
    launch_trace(stream, (unsigned)(hi - lo), kp, a);
}

// One launch of the step kernel for envs [e0, e0 + n) on `stream` (+ the head kernel when bound, + the slice-metrics kernel when on,
// + the trace kernel behind a step while a trace is bound).
template <int MODE>
hipError_t launch_range(ranenv_handle h, KP kp, int e0, int n, hipStream_t stream)
{
    kp.e0 = e0;
    // SE gather mode: tiles replayed from the pool are read through the sidecars; explicit per-step tiles and dense
    // sched_decisions (whole rows are needed) keep the streaming kernel
    const bool gather = MODE != MODE_DENSE && h->se_mode == RANENV_SE_GATHER && kp.se_tiles == nullptr;
    const StepChoice p = step_choice(h, {MODE, kp.n_tti, kp.compact, gather, e0, n, kp.ml_pool != nullptr, kp.env_mask != nullptr, kp.se_tiles != nullptr});
    kp.compact = p.compact;
    if (gather) gather_kp(h, kp);
    KP ks = kp;
    if (p.l.build == SB_MIXED) {
        if (persist_prepare(h, stream, false) != RANENV_OK) return hipErrorUnknown;
        ks.p_list = h->d_plist + (size_t)h->cfg.batch; ks.m_list = h->d_plist; ks.m_counts = h->d_pcount;
    }
    hipEvent_t ev0, ev1;
    const hipError_t pe = prof_events(h, n, MODE == MODE_STEP ? kp.n_tti : 1, &ev0, &ev1);
    if (pe != hipSuccess) return pe;
    const hipError_t le = launch_step_counted(h, p.l, p.grid, p.block, stream, ev0, ev1, ks);
    if (le != hipSuccess) return le;
    if (kp.head_obs || kp.head_reward)
        launch_head(stream, dim3((unsigned)n), dim3((unsigned)h->nslot), kp, (h->kp.acc && h->kp.head_reward) ? h->d_head_acc : nullptr,
                    MODE == MODE_RESET ? 1 : 0);
    if (slice_metrics_on(h))
        launch_slice_metrics(stream, dim3((unsigned)n), dim3((unsigned)h->nslot), kp, h->d_slice_acc, MODE == MODE_RESET ? 1 : 0);
    if (MODE == MODE_STEP && trace_on(h)) launch_trace_range(h, kp, e0, n, stream);
    return hipGetLastError();
}

// May the step that `kp` describes leave the UEs outside every slice alone?  Yes when they get no traffic: the device
// generator never draws for them; a traffic pool is examined once per change of pools / scenarios / episodes (a kernel over
// the episode descriptors and, with auto-reset, over the episode table, then one read-back); explicit per-step traffic is
// not examined at all (full width).
int compact_for(ranenv_handle h, const KP &kp, hipStream_t stream, int *out)
{
    *out = 0;
    // a step that may hand idle UEs packets (explicit traffic, an unexamined or offending pool) leaves them with queues that
    // only full-width steps keep ageing: compact steps stay off until a reset of the whole batch
    if (kp.traffic_bits != nullptr || kp.dense != nullptr) { h->idle_state_clean = false; return RANENV_OK; }
    if (kp.trf_gen) { *out = (h->compact_enabled && h->idle_state_clean) ? 1 : 0; return RANENV_OK; }
    if (!kp.trf_pool) return RANENV_OK;
    if (!h->compact_enabled) return RANENV_OK;
    if (h->idle_check_dirty && stream_capturing(stream)) return RANENV_OK;     // (the examination reads back: a captured step that comes before it runs at full width)
    if (h->idle_check_dirty) {
        if (!h->d_violations && dev_alloc(h, &h->d_violations, 2) != RANENV_OK) return RANENV_E_NOMEM;
        HIP_TRY(h, hipMemsetAsync(h->d_violations, 0, 2 * sizeof(int), stream));
        const int U = h->cfg.n_ues;
        launch_idle_traffic(stream, (unsigned)h->cfg.batch, h->d_episodes, kp.trf_pool, U, TB_ue_slice(h->kp), TB_lane_ue(h->kp), h->d_violations);
        if (h->d_ep_table)
            launch_idle_traffic(stream, (unsigned)h->ep_table_n, h->d_ep_table, kp.trf_pool, U, TB_ue_slice(h->kp), TB_lane_ue(h->kp), h->d_violations + 1);
        int v[2] = {1, 1};
        HIP_TRY(h, hipMemcpyAsync(v, h->d_violations, sizeof(v), hipMemcpyDeviceToHost, stream));
        HIP_TRY(h, hipStreamSynchronize(stream));
        h->pool_idle_zero = v[0] == 0; h->table_idle_zero = h->d_ep_table ? v[1] == 0 : true;
        h->idle_check_dirty = false;
    }
    const bool zero = h->pool_idle_zero && (!h->ar_on || h->table_idle_zero);
    if (!zero) h->idle_state_clean = false;
    *out = (zero && h->compact_enabled && h->idle_state_clean) ? 1 : 0;
    return RANENV_OK;
}

// One TTI of the whole batch.  Without partitions: one launch on the caller's stream.  With partitions: one launch
// per partition on the partition's own stream; `join_in` orders them behind what the caller's stream holds so far
// (inputs), `join_out` orders the caller's stream behind them (outputs).  ranenv_rollout enqueues n TTIs with a join
// only before the first and after the last: partition k's TTI t+1 then follows its own TTI t directly, whatever the
// other partitions are doing -- envs are independent, nothing else orders them.
template <typename Body>      // Body(e0, n, stream) -> hipError_t: what one partition enqueues for one TTI
hipError_t for_partitions(ranenv_handle h, hipStream_t stream, bool join_in, bool join_out, Body body)
{
    hipError_t le = hipSuccess;
    if (h->n_parts <= 1) {
        le = body(0, h->cfg.batch, stream);
        if (le != hipSuccess) return le;
        // RANENV_F_SYNC_CHECK: surface asynchronous kernel faults at the call that caused them
        if (h->cfg.flags & RANENV_F_SYNC_CHECK) return hipStreamSynchronize(stream);
        return hipSuccess;
    }
    join_in = join_in && stream_busy(stream);
    if (join_in) {
        le = hipEventRecord(h->ev_in, stream);
        if (le != hipSuccess) return le;
    }
    // partition 0 runs on the caller's stream itself (a process has few hardware queues -- 4 by default -- and streams
    // beyond them share one, i.e. run one after the other) and is enqueued first: it waits for no event, so the GPU has
    // work ~10 us after the call instead of after the other partitions' event waits; partitions 1.. on the handle's streams
    le = body(h->part_lo[0], h->part_lo[1] - h->part_lo[0], stream);
    if (le != hipSuccess) return le;
    for (int k = 1; k < h->n_parts; k++) {
        hipStream_t ps = h->part_stream[k];
        if (join_in) { le = hipStreamWaitEvent(ps, h->ev_in, 0); if (le != hipSuccess) return le; }
        le = body(h->part_lo[k], h->part_lo[k + 1] - h->part_lo[k], ps);
        if (le != hipSuccess) return le;
        if (join_out) { le = hipEventRecord(h->part_done[k], ps); if (le != hipSuccess) return le; }
    }
    if (join_out)
        for (int k = 1; k < h->n_parts; k++) { le = hipStreamWaitEvent(stream, h->part_done[k], 0); if (le != hipSuccess) return le; }
    if (h->cfg.flags & RANENV_F_SYNC_CHECK) {
        le = hipStreamSynchronize(stream);
        for (int k = 1; k < h->n_parts && le == hipSuccess; k++) le = hipStreamSynchronize(h->part_stream[k]);
        return le;
    }
    return hipSuccess;
}

template <int MODE>
hipError_t launch(ranenv_handle h, const KP &kp, hipStream_t stream)
{
    return for_partitions(h, stream, true, true, [&](int e0, int n, hipStream_t s) { return launch_range<MODE>(h, kp, e0, n, s); });
}

// A call's kernel arguments: the handle's, with every per-call input null, the call's outputs, and one TTI (ranenv_rollout says more)
KP call_kp(ranenv_handle h, float *obs_inter, float *obs_intra, double *reward, uint8_t *done)
{
    KP kp = h->kp;
    kp.env_mask = nullptr; kp.se_tiles = nullptr; kp.scores = nullptr; kp.intra = nullptr; kp.traffic_bits = nullptr; kp.dense = nullptr;
    kp.obs_inter = obs_inter; kp.obs_intra = obs_intra; kp.reward = reward; kp.done = done;
    kp.n_tti = 1;
    return kp;
}

// The reset behind a step (auto-reset): the envs whose episode ended restart.  The step's rewards and done flags stay, those of the
// alternative heads too (head_obs gets the new episode's first observation); full width.
KP reset_behind(ranenv_handle h, KP kp)
{
    kp.env_mask = h->d_ar_mask; kp.reward = nullptr; kp.done = nullptr; kp.head_reward = nullptr; kp.compact = 0;
    return kp;
}

// Auto-reset: the arguments of the advance kernel for this handle's tables and the caller's buffers
AdvanceArgs advance_args(ranenv_handle h, const uint8_t *dev_done, float *obs_inter, float *obs_intra,
                         float *term_obs_inter, float *term_obs_intra, float *term_obs_head)
{
    const int S = h->cfg.n_slices, Us = h->cfg.max_ues_slice;
    AdvanceArgs a;
    a.done = dev_done; a.mask = h->d_ar_mask; a.episodes = h->d_episodes; a.table = h->d_ep_table;
    a.table_first = h->ep_table_first; a.table_n = h->ep_table_n;
    a.episode_no = ST_episode_no(h->kp); a.reset_count = ST_reset_count(h->kp);
    a.initial = h->ar_initial; a.max_ep = h->ar_max; a.random = h->ar_random; a.env_id_base = h->kp.env_id_base; a.seed = h->ar_seed;
    a.obs_inter = obs_inter; a.obs_intra = obs_intra; a.head_obs = h->kp.head_obs;
    a.term_inter = obs_inter ? term_obs_inter : nullptr; a.term_intra = obs_intra ? term_obs_intra : nullptr; a.term_head = term_obs_head;
    a.n_inter = S * 10; a.n_intra = S * (2 * Us + 9); a.n_head = S * 10;
    a.e0 = 0;
    a.cls_flag = h->d_cls_flag;
    a.acc = h->kp.acc; a.ep_acc = h->d_ep_acc; a.ep_n = h->d_ep_n; a.ep_slots = h->ep_slots;
    const bool head_sums = h->kp.acc && h->kp.head_reward && h->d_head_acc && h->d_head_ep_acc;
    a.head_acc = head_sums ? h->d_head_acc : nullptr; a.head_ep_acc = head_sums ? h->d_head_ep_acc : nullptr;
    const bool slice_sums = slice_metrics_on(h) && h->d_slice_ep_acc && h->d_slice_ep_scn;
    a.slice_acc = slice_sums ? h->d_slice_acc : nullptr; a.slice_ep_acc = slice_sums ? h->d_slice_ep_acc : nullptr;
    a.slice_ep_scenario = slice_sums ? h->d_slice_ep_scn : nullptr; a.n_slice = S * RANENV_SLICE_METRIC_COLS;
    return a;
}

int max_steps_of_env(const ranenv *h, int b) { return h->host_max_steps.empty() ? h->cfg.max_steps : h->host_max_steps[(size_t)b]; }

void shadow_steps_add(ranenv_handle h, int lo, int hi, int n, const uint8_t *done, hipStream_t stream)      // n TTIs enqueued for envs [lo, hi)
{
    if (done) h->last_done = done;
    if (!h->sh_valid) return;
    if (stream_capturing(stream)) { h->sh_valid = false; return; }       // (a graph may be replayed any number of times)
    int32_t *s = h->sh_steps.data();
    for (int b = lo; b < hi; b++) s[b] += n;
}
// envs of [lo, hi) whose episode ended at the TTI enqueued last: -1 = unknown (ask the device), else how many
int shadow_due(ranenv_handle h, int lo, int hi, const uint8_t *dev_done, hipStream_t stream)
{
    if (!h->autoreset_shortcut || !h->sh_valid || dev_done == nullptr || dev_done != h->last_done || stream_capturing(stream)) return -1;
    int due = 0;
    for (int b = lo; b < hi; b++) due += h->sh_steps[(size_t)b] >= max_steps_of_env(h, b) ? 1 : 0;
    return due;
}
void shadow_reset_due(ranenv_handle h, int lo, int hi)      // the auto-reset that was just enqueued restarts exactly those envs
{
    if (!h->sh_valid) return;
    for (int b = lo; b < hi; b++) if (h->sh_steps[(size_t)b] >= max_steps_of_env(h, b)) h->sh_steps[(size_t)b] = 0;
}

// ---- persistent rollout (option "persist"), host side ------------------------------------------------------------
hipError_t ensure_streams(ranenv_handle h, size_t n)      // handle-owned streams / events [1, n) exist (index 0 = the caller's stream)
{
    while (h->part_stream.size() < n) {
        hipStream_t st = nullptr; hipEvent_t ev = nullptr;
        hipError_t e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
        if (e != hipSuccess) return e;
        h->part_stream.push_back(st);
        e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
        if (e != hipSuccess) return e;
        h->part_done.push_back(ev);
        ev = nullptr;
        e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
        if (e != hipSuccess) return e;
        h->part_in.push_back(ev);
    }
    if (!h->ev_in) return hipEventCreateWithFlags(&h->ev_in, hipEventDisableTiming);
    return hipSuccess;
}

// The buffers of the work queues (once per handle) and, whenever scenarios / episodes changed, the envs sorted by class.
// Three states of the lists: clean; `pclass_dirty` (the host changed scenarios / episodes, or followed an episode end itself: re-sort);
// `pclass_maybe` (an auto-reset ran: re-sort only if the device's flag says an env restarted -- the host does not read `done`).
// On a CAPTURING stream the sort is enqueued unconditionally and the host's flags stay as they are: what a replay of the graph
// finds in the episode descriptors is not what the host knows now (set_episodes / reset / an eager auto-reset between replays).
int persist_prepare(ranenv_handle h, hipStream_t stream, bool need_host_counts)
{
    const int B = h->cfg.batch, NC = h->nt / WAVE;
    if (!h->d_plist) {
        int cap = 64;
        while (cap < B) cap <<= 1;
        h->p_nclass = NC; h->p_cap = cap;
        if (dev_alloc(h, &h->d_plist, (size_t)NC * B) != RANENV_OK || dev_alloc(h, &h->d_pcount, (size_t)NC) != RANENV_OK ||
            dev_alloc(h, &h->d_pctl, (size_t)NC) != RANENV_OK || dev_alloc(h, &h->d_pslots, (size_t)NC * 8 * (size_t)cap) != RANENV_OK)
            return RANENV_E_NOMEM;
        // the sticky error word lives in host memory the device can write: the host looks at it without a device sync
        HIP_TRY(h, hipHostMalloc((void **)&h->h_perr, sizeof(int), hipHostMallocMapped));
        *h->h_perr = 0;
        HIP_TRY(h, hipHostGetDevicePointer((void **)&h->d_perr_dev, h->h_perr, 0));       // (the same address with unified addressing; asked for, not assumed)
        h->pcount_host.assign((size_t)NC, 0);
        h->pclass_dirty = true;
    }
    const bool capturing = stream_capturing(stream);
    if (capturing && need_host_counts) return fail(h, RANENV_E_STATE, "a persistent rollout reads its class counts back: not inside a stream capture");
    const int one_class = (persist_tiny(h) && h->mix != 2) ? 1 : 0;
    if (h->pclass_dirty || capturing) {
        launch_classify(stream, h->d_episodes, h->d_members, B, NC, one_class, h->d_plist, h->d_pcount, h->d_cls_flag, 1);
        if (!capturing) { h->pclass_dirty = false; h->pclass_maybe = false; h->pcount_host_stale = true; }
    } else if (h->pclass_maybe) {
        launch_classify(stream, h->d_episodes, h->d_members, B, NC, one_class, h->d_plist, h->d_pcount, h->d_cls_flag, 0);
        h->pclass_maybe = false; h->pcount_host_stale = true;
    }
    if (need_host_counts && h->pcount_host_stale) {       // (the persistent launches size their grids by them; mixed launches read them on the device)
        HIP_TRY(h, hipMemcpyAsync(h->pcount_host.data(), h->d_pcount, sizeof(int32_t) * (size_t)NC, hipMemcpyDeviceToHost, stream));
        HIP_TRY(h, hipStreamSynchronize(stream));
        h->pcount_host_stale = false;
    }
    return RANENV_OK;
}

// A wait inside a persistent launch gave up (PersistCtl::abort: every workgroup of that class then drops its env after the
// current chunk, so the envs have advanced different numbers of TTIs).  Seen through the host-visible error word at the next call:
// the queues and cursors are cleared, the persistent rollout is switched off for this handle (the launch-per-chunk rollout
// takes over) and the call fails -- the batch has to be reset.
int persist_check_errors(ranenv_handle h)
{
    if (!h->h_perr || *(volatile int *)h->h_perr == 0) return RANENV_OK;
    HIP_TRY(h, hipDeviceSynchronize());
    HIP_TRY(h, hipMemset(h->d_pctl, 0, sizeof(PersistCtl) * (size_t)h->p_nclass));
    HIP_TRY(h, hipMemset(h->d_pslots, 0, sizeof(unsigned long long) * (size_t)h->p_nclass * 8 * (size_t)h->p_cap));
    *(volatile int *)h->h_perr = 0;
    h->perr_seen++;
    h->persist = 0;
    h->sh_valid = false;           // the envs have advanced different numbers of TTIs: the host no longer knows the step counters
    return fail(h, RANENV_E_STATE, "a persistent rollout launch gave up waiting on its work queue (sticky error word): the envs of the batch "
                "have advanced different numbers of TTIs -- reset the batch; the persistent rollout is now off for this handle "
                "(option persist = 0), its queues were cleared");
}

// One persistent launch per non-empty class for `n_tti` TTIs of every env: the class with the widest blocks on the caller's
// stream (enqueued first: a block of several waves needs that many free slots on one CU), the others on handle-owned streams
// between an event pair.
int persist_launch(ranenv_handle h, KP kp, int n_tti, hipStream_t stream)
{
    const int B = h->cfg.batch, NC = h->p_nclass;
    const StepLaunch l = persist_choice(h, kp.ml_pool != nullptr);      // (the rollout offered its member-lines copy?)
    kp.n_tti = n_tti; kp.compact = 1; kp.e0 = 0;
    // (a chunk is always shorter than the launch, so that the envs reach a chunk end inside it and find the exhausted env cursors
    // there, at different TTIs: without one all workgroups finish together and walk those cursors at once -- DESIGN.md 4.4, "Short
    // rollouts", profiles/r06_ab_log.txt)
    kp.p_chunk = h->persist_chunk < n_tti ? h->persist_chunk : (n_tti > 1 ? n_tti - 1 : 1);
    kp.p_cap = h->p_cap; kp.p_err = h->d_perr_dev;
    if (l.gather) gather_kp(h, kp);
    int &slots_cu = h->p_wave_slots[l.gather ? 1 : 0];
    if (slots_cu == 0) {
        int nb = 0;
        const void *fn = step_kernel_ptr(persist_choice(h, false, true));
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, WAVE, 0) != hipSuccess || nb < 1) { (void)hipGetLastError(); nb = 16; }
        slots_cu = nb;
    }
    long long W = (long long)slots_cu * h->n_cus, demand = 0;
    if (h->persist_grid > 0 && h->persist_grid < W) W = h->persist_grid;
    int n_used = 0;
    for (int c = 0; c < NC; c++) { demand += (long long)h->pcount_host[(size_t)c] * (c + 1); n_used += h->pcount_host[(size_t)c] > 0 ? 1 : 0; }
    if (demand == 0) return RANENV_OK;
    hipError_t e = ensure_streams(h, (size_t)(n_used > 1 ? n_used : 1));
    if (e != hipSuccess) return fail(h, RANENV_E_HIP, "persistent rollout, streams: %s", hipGetErrorString(e));
    // (the other classes' streams pick up behind what the caller's stream holds)
    const bool join_in = n_used > 1 && stream_busy(stream);
    if (join_in) HIP_TRY(h, hipEventRecord(h->ev_in, stream));
    int k = 0;                                     // stream index: 0 = the caller's
    for (int c = NC - 1; c >= 0; c--) {
        const int n = h->pcount_host[(size_t)c];
        if (n == 0) continue;
        long long g = demand <= W ? n : (long long)n * W / demand;
        if (g < 1) g = 1;
        if (g > n) g = n;
        hipStream_t s = k == 0 ? stream : h->part_stream[(size_t)k];
        if (k > 0 && join_in) HIP_TRY(h, hipStreamWaitEvent(s, h->ev_in, 0));
        KP kc = kp;
        // (the envs are NOT bound to workgroups statically, although at B 4096 the grids equal the class sizes: a few dozen workgroups
        // start late, and an env bound to one of those would wait for a whole rollout of somebody else -- DESIGN.md 4.4,
        // profiles/r06_ab_log.txt.  Nor is a launch ever ONE chunk, not even for a batch whose every env has a resident workgroup of its
        // own (configs[1]): see kp.p_chunk above)
        kc.p_list = h->d_plist + (size_t)c * B; kc.p_count = n; kc.p_ctl = h->d_pctl + c;
        kc.p_slots = h->d_pslots + (size_t)c * 8 * (size_t)h->p_cap;
        if (h->persist_inject) {                   // test hook: this launch finds a wait already given up
            const int one = 1;
            HIP_TRY(h, hipMemcpyAsync(&kc.p_ctl->abort, &one, sizeof(int), hipMemcpyHostToDevice, s));      // (the DEVICE then raises the host-visible word)
        }
        hipEvent_t ev0, ev1;
        e = prof_events(h, n, n_tti, &ev0, &ev1);
        if (e != hipSuccess) return fail(h, RANENV_E_HIP, "hipEventCreate(&pe): %s", hipGetErrorString(e));
        const dim3 grid((unsigned)g), block((unsigned)((c + 1) * WAVE));
        e = launch_step_counted(h, l, grid, block, s, ev0, ev1, kc);
        if (e != hipSuccess) return fail(h, RANENV_E_HIP, "persistent rollout launch: %s", hipGetErrorString(e));
        if (k > 0) HIP_TRY(h, hipEventRecord(h->part_done[(size_t)k], s));
        k++;
    }
    for (int j = 1; j < k; j++) HIP_TRY(h, hipStreamWaitEvent(stream, h->part_done[(size_t)j], 0));
    h->persist_inject = 0;
    h->last_rollout_launches += k;
    e = hipGetLastError();
    if (e != hipSuccess) return fail(h, RANENV_E_HIP, "persistent rollout launch: %s", hipGetErrorString(e));
    if (h->cfg.flags & RANENV_F_SYNC_CHECK) HIP_TRY(h, hipStreamSynchronize(stream));
    return RANENV_OK;
}

// Replace the SE gather sidecars by fresh ones for nt tiles (the old ones are released first, behind a device synchronisation), and
// enqueue fill(t0, n) for tiles [t0, t0 + n) in chunks that keep grid.x far below its limit.  A failed fill launch is the caller's to report.
void dev_drop(ranenv_handle h, void *ptr)        // release one of the handle's allocations ahead of ranenv_destroy
{
    if (!ptr) return;
    for (size_t i = 0; i < h->allocs.size(); i++) if (h->allocs[i] == ptr) { h->allocs.erase(h->allocs.begin() + (long)i); break; }
    (void)hipFree(ptr);
}

// A handle-owned scratch buffer of at least `count` elements (contents undefined; an outgrown one is released, nothing is running on it:
// its users end with a stream synchronisation)
template <typename T>
int dev_grow(ranenv_handle h, T **buf, int64_t *cap, int64_t count, const char *what)
{
    if (*buf && *cap >= count) return RANENV_OK;
    dev_drop(h, *buf); *buf = nullptr; *cap = 0;
    void *ptr = nullptr;
    const hipError_t e = hipMalloc(&ptr, (size_t)count * sizeof(T));
    if (e != hipSuccess) return fail(h, RANENV_E_NOMEM, "%s (%.3f GB): %s", what, (double)count * sizeof(T) / 1e9, hipGetErrorString(e));
    h->allocs.push_back(ptr);
    *buf = (T *)ptr; *cap = count;
    return RANENV_OK;
}

template <typename Fill>
int se_sidecars_rebuild(ranenv_handle h, size_t nt, Fill fill)
{
    const int U = h->cfg.n_ues, Rp = (h->cfg.n_rbs + 7) & ~7;
    auto drop = [&](void *ptr) { dev_drop(h, ptr); };
    HIP_TRY(h, hipDeviceSynchronize());
    drop(h->d_se_mean); drop(h->d_se_um); h->d_se_mean = nullptr; h->d_se_um = nullptr;
    void *pm = nullptr, *pu = nullptr;
    hipError_t e = hipMalloc(&pm, nt * (size_t)U * sizeof(double));
    if (e == hipSuccess) e = hipMalloc(&pu, nt * (size_t)U * (size_t)Rp * sizeof(float));
    if (e != hipSuccess) {
        if (pm) (void)hipFree(pm);
        return fail(h, RANENV_E_NOMEM, "SE gather sidecars (%zu tiles: %.2f GB): %s", nt,
                    (double)(nt * (size_t)U * (8 + 4 * (size_t)Rp)) / 1e9, hipGetErrorString(e));
    }
    h->allocs.push_back(pm); h->allocs.push_back(pu);
    h->d_se_mean = (double *)pm; h->d_se_um = (float *)pu; h->se_rp = Rp;
    for (size_t t0 = 0; t0 < nt; t0 += 1u << 20) fill(t0, nt - t0 < (1u << 20) ? nt - t0 : (size_t)(1u << 20));
    return RANENV_OK;
}

// Member lines (ranenv_numeric.hpp, "Member lines"): the lines of one UE's row, in the order of the copy.  The leaves are numpy's
// pairwise ones for ANY row length (the recursion itself, not the kernels' two levels): every leaf a multiple of 8 RBs except that
// the last carries the tail R & 7; a leaf's whole 8-RB groups in chunks of 4, one line each; the tail line last (groups = 0).
struct MemberLine { int leaf, rb0, groups; };
void member_leaves(int lo, int n, std::vector<std::pair<int, int>> &out)
{
    if (n <= 128) { out.push_back({lo, n}); return; }
    int n2 = n / 2; n2 -= n2 % 8;
    member_leaves(lo, n2, out); member_leaves(lo + n2, n - n2, out);
}
std::vector<MemberLine> member_line_plan(int R)
{
    std::vector<std::pair<int, int>> leaves;
    member_leaves(0, R, leaves);
    std::vector<MemberLine> plan;
    for (size_t k = 0; k < leaves.size(); k++) {
        const int G = leaves[k].second >> 3;
        for (int c = 0; 4 * c < G; c++) plan.push_back({(int)k, leaves[k].first + 32 * c, G - 4 * c < 4 ? G - 4 * c : 4});
    }
    if (R & 7) plan.push_back({(int)leaves.size() - 1, R - (R & 7), 0});
    return plan;
}
// ... as the retile kernel takes it (false: more lines than its table holds -- no row length ranenv_create admits)
bool member_line_table(int R, MemberLineTable *tb)
{
    const std::vector<MemberLine> plan = member_line_plan(R);
    if (plan.size() > (size_t)MEMBER_LINES_MAX) return false;
    *tb = MemberLineTable{};
    tb->lines = (int)plan.size(); tb->tail = R & 7;
    for (size_t l = 0; l < plan.size(); l++) { tb->rb0[l] = plan[l].rb0; tb->groups[l] = plan[l].groups; }
    return true;
}
// The whole 8-RB groups of the leaf [lo, lo + n), n <= 128, from the lines at `line` on (advanced): a cluster's part of a leaf -- per
// accumulator j the four elements of a line one after the other, then the tree (+0.0 for a leaf without a whole group)
void member_leaf_groups(const float *&line, int lo, int n, unsigned s, unsigned c, double &fr, double &gr)
{
    auto in = [&](int r) { return ((unsigned)r - s) < c ? 1.0 : 0.0; };
    double f[8], g[8];
    for (int j = 0; j < 8; j++) { f[j] = 0.0; g[j] = 0.0; }
    const int G = n >> 3;
    for (int c4 = 0; 4 * c4 < G; c4++, line += 32)
        for (int j = 0; j < 8; j++)
            for (int k = 0; k < 4; k++) {
                const double d = (double)line[4 * j + k];
                f[j] += d;
                g[j] = std::fma(d, in(lo + 8 * (4 * c4 + k) + j), g[j]);
            }
    fr = ((f[0] + f[1]) + (f[2] + f[3])) + ((f[4] + f[5]) + (f[6] + f[7]));
    gr = ((g[0] + g[1]) + (g[2] + g[3])) + ((g[4] + g[5]) + (g[6] + g[7]));
}
// `full` / `part` of rows [lo, lo + n) from the lines at `line` on (advanced), added in the kernel's order: per accumulator j the four
// elements of a line one after the other, the leaf's tree, the tail sequentially, the halves as numpy's recursion folds them
void member_lines_pairwise(const float *&line, int lo, int n, unsigned s, unsigned c, double &full, double &part)
{
    if (n > 128) {
        int n2 = n / 2; n2 -= n2 % 8;
        double f1, g1, f2, g2;
        member_lines_pairwise(line, lo, n2, s, c, f1, g1); member_lines_pairwise(line, lo + n2, n - n2, s, c, f2, g2);
        full = f1 + f2; part = g1 + g2;
        return;
    }
    auto in = [&](int r) { return ((unsigned)r - s) < c ? 1.0 : 0.0; };
    const int G = n >> 3, tail = n & 7;
    double fr, gr;
    member_leaf_groups(line, lo, n, s, c, fr, gr);
    if (tail > 0) {
        for (int k = 0; k < tail; k++) { const double d = (double)line[k]; fr += d; gr = std::fma(d, in(lo + 8 * G + k), gr); }
        line += 32;
    }
    full = fr; part = gr;
}

// The packed copy of a tile (ranenv_numeric.hpp, "Member lines"): [U][nlw][32] whole-group lines, then the tail block [U][8] where
// R mod 8 != 0, the tile rounded up to whole lines.  false: more lines than the retile kernel's table holds.
struct PackedLayout { int nlw; long long block_off, tile_bytes; };
static bool member_lines_packed_layout(int U, int R, PackedLayout *pk, MemberLineTable *tb)
{
    if (!member_line_table(R, tb)) return false;
    const int tail = R & 7;
    pk->nlw = tb->lines - (tail ? 1 : 0);
    pk->block_off = (long long)U * pk->nlw * 128;
    pk->tile_bytes = (pk->block_off + (tail ? 32ll * U : 0) + 127) / 128 * 128;
    return true;
}

// tiles [0, n_tiles) of a pool -> the packed copy at dst, in bursts (one launch writes walk lines, block and padding)
static void retile_member_lines_packed(hipStream_t stream, const float *pool, long long pool_stride, int quad, float *dst, long long n_tiles, int U, int R,
                                       const MemberLineTable &tb, const PackedLayout &pk)
{
    const long long burst = 1ll << 16, f4 = pk.tile_bytes / 16;
    for (long long t0 = 0; t0 < n_tiles; t0 += burst) {
        const long long n = n_tiles - t0 < burst ? n_tiles - t0 : burst;
        long long blocks = (n * f4 + 255) / 256;
        if (blocks > 256 * 64) blocks = 256 * 64;
        launch_se_retile_member_lines(stream, (unsigned)blocks, pool + (size_t)t0 * (size_t)pool_stride, pool_stride, quad, dst + (size_t)t0 * (size_t)(pk.tile_bytes / 4),
                                      n, U, R, tb, f4);
    }
}

// The member-lines copy for the pool as it is bound now: there (true), or not and not to be built here -- no pool, a failed allocation
// earlier, a capturing stream.  Built once per binding, in bursts like the sidecars, between a device and a stream synchronisation:
// launches on other streams (the partitions' own) read it.  A failed allocation raises no error: the variant stays off for the handle.
bool member_lines_ready(ranenv_handle h, hipStream_t stream)
{
    if (h->ml_valid) return true;
    MemberLineTable tb; PackedLayout pk;
    if (h->ml_failed || !h->kp.se_pool || h->se_tiles_n < 1 || stream_capturing(stream) || !member_lines_packed_layout(h->cfg.n_ues, h->cfg.n_rbs, &pk, &tb))
        return false;
    const int U = h->cfg.n_ues, R = h->cfg.n_rbs;
    const long long stride = pk.tile_bytes / 4;
    const int64_t count = h->se_tiles_n * stride;
    if (hipDeviceSynchronize() != hipSuccess) { (void)hipGetLastError(); return false; }
    if (!(h->d_ml && h->ml_cap >= count)) {
        dev_drop(h, h->d_ml); h->d_ml = nullptr; h->ml_cap = 0;
        void *ptr = nullptr;
        if (hipMalloc(&ptr, (size_t)count * sizeof(float)) != hipSuccess) { (void)hipGetLastError(); h->ml_failed = true; return false; }
        h->allocs.push_back(ptr);
        h->d_ml = (float *)ptr; h->ml_cap = count;
    }
    retile_member_lines_packed(stream, h->kp.se_pool, (long long)h->kp.se_stride, h->kp.se_quad, h->d_ml, (long long)h->se_tiles_n, U, R, tb, pk);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) { (void)hipGetLastError(); h->ml_failed = true; return false; }
    h->ml_stride = stride; h->ml_valid = true;
    return true;
}

// Tuning / debug options (include/ranenv.h, "Options"): ONE table of the keys behind ranenv_set_option / _get_option, and ONE place where the
// process environment is read (ranenv_create -> apply_env_options: RANENV_<KEY IN CAPITALS>=value presets the same
// options for handles created afterwards; the test suite and the A/B tools run whole passes under them).
// None of them changes a result: they select a launch schedule or a build of the step kernel.
struct Option {
    const char *key;
    bool env;                                   // preset from RANENV_<KEY IN CAPITALS>
    int (*set)(ranenv_handle, long long);       // stores a value, clamped / normalised, or refuses it
    long long (*get)(ranenv_handle);            // reads it back (null: not readable)
};
using H = ranenv_handle;
const Option options[] = {
    {"compact", true, [](H h, long long v) { h->compact_enabled = v != 0; return 0; }, [](H h) -> long long { return h->compact_enabled ? 1 : 0; }},
    {"fuse", true, [](H h, long long v) { h->fuse = v < 0 ? 0 : (v > 64 ? 64 : (int)v); return 0; }, [](H h) -> long long { return h->fuse; }},
    {"row_width", true, [](H h, long long v) {
         const int m = h->cfg.n_slices > h->cfg.max_ues_slice ? h->cfg.n_slices : h->cfg.max_ues_slice;
         if (!((v == 8 || v == 10 || v == 16) && v >= m))
             return fail(h, RANENV_E_INVALID, "row_width must be 8, 10 or 16 and >= max(S, Us) = %d", m);
         h->np = (int)v;
         return 0;
     }, [](H h) -> long long { return h->np; }},
    {"small_batch", true, [](H h, long long v) { h->small_batch = v != 0; return 0; }, [](H h) -> long long { return h->small_batch ? 1 : 0; }},
    {"tiny_step", true, [](H h, long long v) { h->tiny_step = v != 0 ? 1 : 0; return 0; }, [](H h) -> long long { return h->tiny_step; }},
    {"persist", true, [](H h, long long v) { h->persist = v < 0 ? -1 : (v != 0 ? 1 : 0); return 0; }, [](H h) -> long long { return h->persist; }},
    {"persist_chunk", true, [](H h, long long v) { h->persist_chunk = v < 1 ? 1 : (v > 1000 ? 1000 : (int)v); return 0; },
     [](H h) -> long long { return h->persist_chunk; }},
    {"persist_grid", true, [](H h, long long v) { h->persist_grid = v < 0 ? 0 : (int)v; return 0; }, [](H h) -> long long { return h->persist_grid; }},
    {"pack", true, [](H h, long long v) { h->pack = v != 0; return 0; }, [](H h) -> long long { return h->pack ? 1 : 0; }},
    {"mix", true, [](H h, long long v) { h->mix = v < 0 ? 0 : (v > 2 ? 2 : (int)v); h->pclass_dirty = true; return 0; },
     [](H h) -> long long { return h->mix; }},
    // test hook, see persist_check_errors
    {"persist_inject_abort", false, [](H h, long long v) { h->persist_inject = v != 0 ? 1 : 0; return 0; }, nullptr},
    {"collect_split", true, [](H h, long long v) { h->collect_split = v < 0 ? -1 : (v != 0 ? 1 : 0); return 0; }, [](H h) -> long long { return h->collect_split; }},
    {"autoreset_shortcut", true, [](H h, long long v) { h->autoreset_shortcut = v != 0 ? 1 : 0; return 0; },
     [](H h) -> long long { return h->autoreset_shortcut; }},
    {"member_lines", true, [](H h, long long v) { h->member_lines = v < 0 ? -1 : (v != 0 ? 1 : 0); return 0; }, [](H h) -> long long { return h->member_lines; }},
    // (kept in the handle's argument block: every call's KP is a copy of it)
    {"lean_tail", true, [](H h, long long v) { h->kp.lean_tail = v != 0 ? 1 : 0; return 0; }, [](H h) -> long long { return h->kp.lean_tail; }},
    {"lean_state", true, [](H h, long long v) { h->kp.lean_state = v != 0 ? 1 : 0; return 0; }, [](H h) -> long long { return h->kp.lean_state; }},
};

const Option *find_option(const std::string &k)
{
    for (const Option &o : options) if (k == o.key) return &o;
    return nullptr;
}

// "fuse_first0" ... "fuse_first9": the index, else -1
int fuse_first_index(const std::string &k)
{
    return k.rfind("fuse_first", 0) == 0 && k.size() == 11 && k[10] >= '0' && k[10] <= '9' ? k[10] - '0' : -1;
}

int set_option(ranenv_handle h, const std::string &k, long long v)
{
    if (const Option *o = find_option(k)) return o->set(h, v);
    const int i = fuse_first_index(k);
    if (i < 0) return fail(h, RANENV_E_INVALID, "unknown option '%s'", k.c_str());
    if (h->fuse_first.size() <= (size_t)i) h->fuse_first.resize((size_t)i + 1, 0);
    h->fuse_first[(size_t)i] = v < 0 ? 0 : (int)v;
    return RANENV_OK;
}

void apply_env_options(ranenv_handle h)
{
    for (const Option &o : options) {
        if (!o.env) continue;
        std::string name = "RANENV_";
        for (const char *c = o.key; *c; c++) name += (char)toupper((unsigned char)*c);
        if (const char *v = getenv(name.c_str())) (void)o.set(h, atoll(v));      // (an unusable value is ignored)
    }
    if (const char *ff = getenv("RANENV_FUSE_FIRST")) {      // a list: a,b,c = partitions 0, 1, 2
        int i = 0;
        for (const char *c = ff; *c && i < 10; i++) {
            (void)set_option(h, std::string("fuse_first") + (char)('0' + i), atoll(c));
            while (*c && *c != ',') c++;
            if (*c) c++;
        }
    }
}

}  // namespace

extern "C" {

const char *ranenv_last_error(ranenv_handle h) { return h ? h->err.c_str() : g_last_error.c_str(); }
int ranenv_abi_version(void) { return RANENV_ABI_VERSION; }

int ranenv_create(const ranenv_config *cfg, ranenv_handle *out)
{
    if (!cfg || !out) return fail(nullptr, RANENV_E_INVALID, "null argument");
    *out = nullptr;
    if (cfg->abi_version != RANENV_ABI_VERSION) return fail(nullptr, RANENV_E_INVALID, "abi_version %d != %d", cfg->abi_version, RANENV_ABI_VERSION);
    const int S = cfg->n_slices, U = cfg->n_ues, R = cfg->n_rbs, Us = cfg->max_ues_slice;
    if (cfg->batch < 1 || S < 1 || S > GRP || U < 1 || U > CORE_NT || R < 1 || R > 512 || Us < 1 || Us > GRP ||
        cfg->rbs_per_rbg < 1 || cfg->rbs_per_rbg > R || cfg->hist_depth < 1 || cfg->hist_depth > 64 ||
        cfg->max_age_cap < 1 || cfg->max_age_cap > 65000 || cfg->max_steps < 1 || cfg->n_scenarios < 1)
        return fail(nullptr, RANENV_E_INVALID,
                    "unsupported sizes: need 1<=S<=16, 1<=U<=256, 1<=R<=512, 1<=Us<=16, 1<=G<=R, 1<=hist_depth<=64");
    // (the kernels divide by these with the guard-free sequence of ddiv: positive NORMAL numbers of moderate magnitude only)
    auto sane = [](double v) { return v >= 1e-30 && v <= 1e30; };
    if (!sane(cfg->bandwidth_hz)) return fail(nullptr, RANENV_E_INVALID, "bandwidth_hz must be a finite positive number in [1e-30, 1e30]");
    if (cfg->flags & ~(RANENV_F_CLEAR_HISTORY_ON_RESET | RANENV_F_NO_RAW_OUTPUT | RANENV_F_SYNC_CHECK | RANENV_F_SCALE_PER_ELEMENT))
        return fail(nullptr, RANENV_E_INVALID, "unknown bits in flags (0x%x)", (unsigned)cfg->flags);
    if (!sane(cfg->norm_traffic) || !sane(cfg->norm_ues) || !sane(cfg->norm_se))
        return fail(nullptr, RANENV_E_INVALID, "norm_traffic, norm_ues, norm_se (the observation's normalisers, agents/ib_sched.py:166-168) must be finite positive numbers in [1e-30, 1e30]");
    if (R > 128) {   // the row reduction follows numpy's pairwise split two levels deep: every leaf must be <= 128 RBs
        int n2 = R / 2; n2 -= n2 % 8;
        const int halves[2] = {n2, R - n2};
        for (int k = 0; k < 2; k++) {
            int a = halves[k], b = 0;
            if (a > 128) { int hh = a / 2; hh -= hh % 8; b = a - hh; a = hh; }
            if (a > 128 || b > 128)
                return fail(nullptr, RANENV_E_INVALID, "n_rbs %d needs a third level of numpy's pairwise split (a leaf of %d RBs): "
                            "supported are R <= 488 and the R in [489,512] whose quarters stay <= 128", R, a > b ? a : b);
        }
    }
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) return fail(nullptr, RANENV_E_HIP, "no HIP device: %s", hipGetErrorString(e));
    if (cfg->device < 0 || cfg->device >= ndev) return fail(nullptr, RANENV_E_INVALID, "device %d out of range (%d)", cfg->device, ndev);
    ranenv_handle h = new (std::nothrow) ranenv();
    if (!h) return fail(nullptr, RANENV_E_NOMEM, "out of host memory");
    h->cfg = *cfg;
    HIP_TRY(h, hipSetDevice(cfg->device));
    const size_t B = (size_t)cfg->batch, NS = (size_t)cfg->n_scenarios, D = (size_t)cfg->hist_depth;
    const size_t L = (size_t)cfg->max_age_cap + 1;
    KP &kp = h->kp;
    memset(&kp, 0, sizeof(kp));
    kp.B = cfg->batch; kp.S = S; kp.U = U; kp.R = R; kp.G = cfg->rbs_per_rbg; kp.Us = Us; kp.D = cfg->hist_depth;
    kp.L = (int)L; kp.max_steps = cfg->max_steps; kp.flags = cfg->flags; kp.T = R / cfg->rbs_per_rbg;
    kp.policy = RANENV_POLICY_MARR; kp.fixed_intra = RANENV_INTRA_RR;
    kp.bw_hz = cfg->bandwidth_hz; kp.bw_per_rb = cfg->bandwidth_hz / (double)R; kp.over = cfg->overfulfill;
    kp.norm_traffic = cfg->norm_traffic; kp.norm_ues = cfg->norm_ues; kp.norm_se = cfg->norm_se;
    kp.lean_tail = 1;
    kp.lean_state = 1;
    int rc = RANENV_OK;
#define ALLOC(field, count) if (rc == RANENV_OK) rc = dev_alloc(h, &field, (count))
    const size_t NSL = (size_t)S * GRP;
    kp.BU = (long long)(B * U); kp.NSU = (long long)(NS * U); kp.NSL = (long long)(NS * NSL);
    ALLOC(kp.tab.slice_i32, NS * S * 8); ALLOC(kp.tab.slice_f64, NS * S * 2);
    ALLOC(kp.tab.param_i32, 2 * NS * S * 6); ALLOC(kp.tab.param_f64, 2 * NS * S * 3);
    ALLOC(kp.tab.slice_ues, NS * S * Us); ALLOC(kp.tab.slice_usecase, NS * S);
    ALLOC(kp.tab.ue, (size_t)N_TUE * NS * U); ALLOC(kp.tab.slot, 3 * NS * NSL);
    ALLOC(kp.st.u4, (size_t)N_U4 * B * U); ALLOC(kp.st.u8, (size_t)N_U8 * B * U); ALLOC(kp.st.b4, (size_t)N_B4 * B);
    ALLOC(kp.st.age_ring, B * L * U); ALLOC(kp.st.ring_sent, B * D * U); ALLOC(kp.st.ring_drop, B * D * U);
    ALLOC(kp.st.mask_inter, B * S); ALLOC(kp.st.mask_intra, B * S * Us); ALLOC(kp.st.policy_scores, B * S);
    ALLOC(h->d_episodes, B); ALLOC(h->d_ar_mask, B); ALLOC(h->d_members, NS); ALLOC(h->d_cls_flag, 1);
#undef ALLOC
    if (rc != RANENV_OK) { std::string m = h->err; ranenv_destroy(h); g_last_error = m; return rc; }
    kp.episodes = h->d_episodes;
    h->nt = (U + WAVE - 1) / WAVE * WAVE;               // step kernel: one lane per UE ...
    if (h->nt < (S * 8 + WAVE - 1) / WAVE * WAVE) h->nt = (S * 8 + WAVE - 1) / WAVE * WAVE;   // ... and per slice-table word
    h->nslot = (S * GRP + WAVE - 1) / WAVE * WAVE;      // head kernel: one lane per slot
    {
        const int m = S > Us ? S : Us;
        h->np = m <= 8 ? 8 : (m <= 10 ? 10 : 16);
    }
    {   // fail at create, not at the first step, when the code object has no gfx950 image
        hipFuncAttributes fa;
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, cfg->device) == hipSuccess && prop.multiProcessorCount > 0) {
            h->n_cus = prop.multiProcessorCount;
            h->small_batch = (long long)cfg->batch <= 8ll * prop.multiProcessorCount;
        }
        e = hipFuncGetAttributes(&fa, step_kernel_ptr(step_choice(h, {MODE_RESET, 1, 0, false, 0, cfg->batch}).l));      // (a reset of the whole batch)
        if (e != hipSuccess) {
            ranenv_destroy(h);
            return fail(nullptr, RANENV_E_HIP, "no usable gfx950 kernel image (hipFuncGetAttributes: %s)", hipGetErrorString(e));
        }
    }
    apply_env_options(h);
    *out = h;
    return RANENV_OK;
}

int ranenv_set_option(ranenv_handle h, const char *key, int64_t value)
{
    if (!h || !key) return fail(h, RANENV_E_INVALID, "null argument");
    return set_option(h, key, (long long)value);
}

int ranenv_get_option(ranenv_handle h, const char *key, int64_t *value)
{
    if (!h || !key || !value) return fail(h, RANENV_E_INVALID, "null argument");
    const std::string k(key);
    const Option *o = find_option(k);
    if (o && o->get) *value = o->get(h);
    else if (k.rfind("persist_stat_", 0) == 0) {      // keep / push / pop / fresh / idle_polls, summed over classes and XCDs
        static const char *const names[] = {"keep", "push", "pop", "fresh", "idle_polls"};
        int which = -1;
        for (int i = 0; i < 5; i++) if (k == std::string("persist_stat_") + names[i]) which = i;
        if (which < 0) return fail(h, RANENV_E_INVALID, "unknown option '%s'", key);
        long long tot = 0;
        if (h->d_pctl) {
            HIP_TRY(h, hipSetDevice(h->cfg.device)); HIP_TRY(h, hipDeviceSynchronize());
            std::vector<PersistCtl> ctl((size_t)h->p_nclass);
            HIP_TRY(h, hipMemcpy(ctl.data(), h->d_pctl, sizeof(PersistCtl) * ctl.size(), hipMemcpyDeviceToHost));
            for (auto &c : ctl) for (int x = 0; x < 8; x++) tot += (long long)c.stat[x][which];
        }
        *value = tot;
    }
    else if (k == "persist_errors") {          // persistent launches that gave up a wait: reported so far + pending (0 in every correct run)
        int v = 0;
        if (h->h_perr) { HIP_TRY(h, hipSetDevice(h->cfg.device)); HIP_TRY(h, hipDeviceSynchronize()); v = *(volatile int *)h->h_perr != 0 ? 1 : 0; }
        *value = h->perr_seen + v;
    }
    else if (k == "last_rollout_persistent") *value = h->last_rollout_persistent;      // what the last ranenv_rollout call ran:
    else if (k == "last_rollout_launches") *value = h->last_rollout_launches;          // 1 = persistent work-queue launches; step-kernel launches enqueued
    else if (k == "last_rollout_member_lines") *value = h->last_rollout_member_lines;  // 1 = its step launches read the member-lines copy
    else if (k == "last_rollout_kept_state_ttis") *value = h->last_rollout_kept_state_ttis;      // TTIs its step launches enqueued without the per-UE state's stores
    else if (k == "last_rollout_lean_ttis") *value = h->last_rollout_lean_ttis;        // TTIs its step launches enqueued without the observation tail
    else if (k.rfind("step_launches_", 0) == 0) {      // MODE_STEP launches per build since ranenv_create; "..._many": those of several TTIs
        std::string b = k.substr(14);
        const bool many_only = b.size() > 5 && b.compare(b.size() - 5, 5, "_many") == 0;
        if (many_only) b.resize(b.size() - 5);
        int which = -1;
        for (int i = 0; i < N_STEP_BUILDS; i++) if (b == step_build_names[i]) which = i;
        if (which < 0) return fail(h, RANENV_E_INVALID, "unknown option '%s'", key);
        *value = (int64_t)(h->step_launches[which][1] + (many_only ? 0 : h->step_launches[which][0]));
    }
    else if (const int i = fuse_first_index(k); i >= 0) *value = (size_t)i < h->fuse_first.size() ? h->fuse_first[(size_t)i] : 0;
    else return fail(h, RANENV_E_INVALID, "unknown option '%s'", key);
    return RANENV_OK;
}

int ranenv_destroy(ranenv_handle h)
{
    if (!h) return RANENV_OK;
    (void)hipSetDevice(h->cfg.device);
    (void)hipDeviceSynchronize();
    for (auto &e : h->prof_ev) if (e) (void)hipEventDestroy(e);
    for (auto &e : h->part_done) if (e) (void)hipEventDestroy(e);
    for (auto &e : h->part_in) if (e) (void)hipEventDestroy(e);
    for (auto &st : h->part_stream) if (st) (void)hipStreamDestroy(st);
    if (h->ev_in) (void)hipEventDestroy(h->ev_in);
    for (void *p : h->allocs) (void)hipFree(p);
    if (h->rows.d_chunks) (void)hipFree(h->rows.d_chunks);
    if (h->rows.d_base) (void)hipFree(h->rows.d_base);
    if (h->h_perr) (void)hipHostFree(h->h_perr);
    delete h;
    return RANENV_OK;
}

int ranenv_load_scenarios(ranenv_handle h, int32_t first, int32_t count, const ranenv_scenario_tables *t, void *stream_)
{
    if (!h || !t) return fail(h, RANENV_E_INVALID, "null argument");
    const int S = h->cfg.n_slices, U = h->cfg.n_ues, Us = h->cfg.max_ues_slice;
    if (first < 0 || count < 1 || first + count > h->cfg.n_scenarios) return fail(h, RANENV_E_INVALID, "scenario rows [%d,%d) outside pool of %d", first, first + count, h->cfg.n_scenarios);
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const size_t n = (size_t)count;
    // validate + pack on the host
    std::vector<int32_t> si(n * S * 8), pi(n * S * 6), bmi(n * S * 6);
    std::vector<double> sf(n * S * 2), pf(n * S * 3), bmf(n * S * 3);
    for (size_t i = 0; i < n * S; i++) {
        const int nues = t->slice_nues[i], npar = t->slice_nparams[i], srt = t->sorted_slices[i];
        if (nues < 0 || nues > Us) return fail(h, RANENV_E_INVALID, "slice_nues %d outside [0,%d]", nues, Us);
        if (npar < 0 || npar > 3) return fail(h, RANENV_E_INVALID, "slice_nparams %d outside [0,3]", npar);
        if (srt < 0 || srt >= S) return fail(h, RANENV_E_INVALID, "sorted_slices entry %d outside [0,%d)", srt, S);
        if (t->slice_has_req[i] && nues > 0 && (t->slice_message_size[i] <= 0 || t->slice_buffer_size[i] <= 0))
            return fail(h, RANENV_E_INVALID, "message_size and buffer_size must be positive");
        int32_t *d = &si[i * 8];
        d[0] = t->slice_active[i]; d[1] = t->slice_has_req[i]; d[2] = nues; d[3] = t->slice_buffer_size[i];
        d[4] = t->slice_buffer_latency[i]; d[5] = t->slice_message_size[i]; d[6] = npar; d[7] = srt;
        sf[i * 2] = t->slice_priority[i]; sf[i * 2 + 1] = t->slice_traffic[i];
        for (int k = 0; k < 3; k++) {
            const int m = t->param_metric[i * 3 + k], op = t->param_op[i * 3 + k];
            if (k < npar && (m < 0 || m > 2 || op < 0 || op > 4)) return fail(h, RANENV_E_INVALID, "bad intent parameter (metric %d, op %d)", m, op);
            pi[(i * 3 + k) * 2] = m; pi[(i * 3 + k) * 2 + 1] = op; pf[i * 3 + k] = t->param_value[i * 3 + k];
        }
        // the same by metric, which is the table the step kernel reads.  intent_drift_calc ACCUMULATES once per parameter (agents/common.py:
        // `observations[...] +=`), so two parameters on one metric would add up there while one by-metric entry holds a single (op, value):
        // such a table is refused (include/ranenv.h), as ScenarioTables.set_from_reference refuses the request it would come from
        for (int m = 0; m < 3; m++) { bmi[(i * 3 + m) * 2] = 0; bmi[(i * 3 + m) * 2 + 1] = 0; bmf[i * 3 + m] = 1.0; }
        for (int k = 0; k < npar; k++) {
            const int m = t->param_metric[i * 3 + k];
            if (bmi[(i * 3 + m) * 2]) return fail(h, RANENV_E_INVALID, "scenario %zu slice %zu declares metric %d twice: one parameter per metric and slice", i / S, i % S, m);
            bmi[(i * 3 + m) * 2] = 1; bmi[(i * 3 + m) * 2 + 1] = t->param_op[i * 3 + k]; bmf[i * 3 + m] = t->param_value[i * 3 + k];
        }
        for (int k = 0; k < nues; k++) {
            const int ue = t->slice_ues[i * Us + k];
            if (ue < 0 || ue >= U) return fail(h, RANENV_E_INVALID, "slice_ues entry %d outside [0,%d)", ue, U);
        }
    }
    for (size_t i = 0; i < n; i++) {   // sorted_slices must be a permutation
        std::vector<char> seen(S, 0);
        for (int s = 0; s < S; s++) seen[t->sorted_slices[i * S + s]] = 1;
        for (int s = 0; s < S; s++) if (!seen[s]) return fail(h, RANENV_E_INVALID, "sorted_slices row %zu is not a permutation", i);
    }
    for (size_t i = 0; i < n * U; i++) {
        if (t->ue_pkt_size[i] <= 0 || t->ue_max_pkts[i] <= 0) return fail(h, RANENV_E_INVALID, "ue_pkt_size / ue_max_pkts must be positive");
        if (t->ue_max_age[i] < 0 || t->ue_max_age[i] > h->cfg.max_age_cap) return fail(h, RANENV_E_INVALID, "ue_max_age %d outside [0, max_age_cap=%d]", t->ue_max_age[i], h->cfg.max_age_cap);
        if (t->ue_slice[i] < -1 || t->ue_slice[i] >= S) return fail(h, RANENV_E_INVALID, "ue_slice %d outside [-1,%d)", t->ue_slice[i], S);
        if (t->ue_pos[i] < 0 || t->ue_pos[i] >= Us) return fail(h, RANENV_E_INVALID, "ue_pos %d outside [0,%d)", t->ue_pos[i], Us);
    }
    // slot tables: slot = slice*16 + position -> UE id and that UE's buffer parameters
    const size_t NSL = (size_t)S * GRP;
    std::vector<int32_t> sue(n * NSL, -1), smp(n * NSL, 1), spk(n * NSL, 1);
    for (size_t i = 0; i < n; i++)
        for (int sl = 0; sl < S; sl++)
            for (int k = 0; k < t->slice_nues[i * S + sl]; k++) {
                const int ue = t->slice_ues[(i * S + sl) * Us + k];
                const size_t o = i * NSL + (size_t)sl * GRP + k;
                if (t->ue_slice[i * U + ue] != sl || t->ue_pos[i * U + ue] != k)
                    return fail(h, RANENV_E_INVALID, "scenario %zu: ue_slice/ue_pos disagree with slice_ues", i);
                sue[o] = ue; smp[o] = t->ue_max_pkts[i * U + ue]; spk[o] = t->ue_pkt_size[i * U + ue];
            }
    // per-UE tables in lane order: a scenario's UEs in slices first (ascending UE id), the idle ones behind
    std::vector<int32_t> lt[N_TUE];
    for (auto &v : lt) v.resize(n * (size_t)U);
    for (size_t i = 0; i < n; i++) {
        int l = 0;
        for (int pass = 0; pass < 2; pass++)
            for (int ue = 0; ue < U; ue++) {
                const size_t o = i * U + ue;
                if ((t->ue_slice[o] >= 0) != (pass == 0)) continue;
                const size_t d = i * U + (size_t)l++;
                lt[0][d] = t->ue_slice[o]; lt[1][d] = t->ue_pos[o]; lt[2][d] = t->ue_pkt_size[o];
                lt[3][d] = t->ue_max_pkts[o]; lt[4][d] = t->ue_max_age[o]; lt[5][d] = ue;
            }
    }
    h->idle_check_dirty = true;                 // which UEs are idle changed: traffic traces are re-examined before compact steps
    if (h->members_host.size() != (size_t)h->cfg.n_scenarios) h->members_host.assign((size_t)h->cfg.n_scenarios, 0);
    for (size_t i = 0; i < n; i++) {
        int m = 0;
        for (int ue = 0; ue < U; ue++) m += t->ue_slice[i * U + ue] >= 0 ? 1 : 0;
        h->members_host[(size_t)first + i] = m;
    }
    h->pclass_dirty = true;
    const size_t f = (size_t)first;
    const Tables &d = h->kp.tab;
    const KP &k = h->kp;
#define PUT(dst, src, elems, type) HIP_TRY(h, hipMemcpyAsync((dst), (src), (elems) * sizeof(type), hipMemcpyHostToDevice, stream))
    PUT(d.slice_i32 + f * S * 8, si.data(), n * S * 8, int32_t);
    PUT(d.slice_f64 + f * S * 2, sf.data(), n * S * 2, double);
    PUT(d.param_i32 + f * S * 6, pi.data(), n * S * 6, int32_t);
    PUT(d.param_f64 + f * S * 3, pf.data(), n * S * 3, double);
    PUT(d.param_i32 + ((size_t)h->cfg.n_scenarios + f) * S * 6, bmi.data(), n * S * 6, int32_t);
    PUT(d.param_f64 + ((size_t)h->cfg.n_scenarios + f) * S * 3, bmf.data(), n * S * 3, double);
    PUT(d.slice_ues + f * S * Us, t->slice_ues, n * S * Us, int32_t);
    PUT(TB_ue_slice(k) + f * U, lt[0].data(), n * U, int32_t);
    PUT(TB_ue_pos(k) + f * U, lt[1].data(), n * U, int32_t);
    PUT(TB_ue_pkt_size(k) + f * U, lt[2].data(), n * U, int32_t);
    PUT(TB_ue_max_pkts(k) + f * U, lt[3].data(), n * U, int32_t);
    PUT(TB_ue_max_age(k) + f * U, lt[4].data(), n * U, int32_t);
    PUT(TB_lane_ue(k) + f * U, lt[5].data(), n * U, int32_t);
    {   // set 1: lane = UE
        const size_t set1 = (size_t)6 * (size_t)k.NSU;
        std::vector<int32_t> ident(n * (size_t)U);
        for (size_t i = 0; i < ident.size(); i++) ident[i] = (int32_t)(i % (size_t)U);
        PUT(TB_ue_slice(k) + set1 + f * U, t->ue_slice, n * U, int32_t);
        PUT(TB_ue_pos(k) + set1 + f * U, t->ue_pos, n * U, int32_t);
        PUT(TB_ue_pkt_size(k) + set1 + f * U, t->ue_pkt_size, n * U, int32_t);
        PUT(TB_ue_max_pkts(k) + set1 + f * U, t->ue_max_pkts, n * U, int32_t);
        PUT(TB_ue_max_age(k) + set1 + f * U, t->ue_max_age, n * U, int32_t);
        PUT(TB_lane_ue(k) + set1 + f * U, ident.data(), n * U, int32_t);
        HIP_TRY(h, hipStreamSynchronize(stream));          // `ident` dies here
    }
    PUT(h->d_members + f, h->members_host.data() + f, n, int32_t);
    PUT(TB_slot_ue(k) + f * NSL, sue.data(), n * NSL, int32_t);
    PUT(TB_slot_mp(k) + f * NSL, smp.data(), n * NSL, int32_t);
    PUT(TB_slot_pk(k) + f * NSL, spk.data(), n * NSL, int32_t);
#undef PUT
    HIP_TRY(h, hipStreamSynchronize(stream));  // staging vectors die at return
    h->have_scenarios = true;
    if (h->slice_traffic.size() != NS_all(h)) { h->slice_traffic.assign(NS_all(h), 0.0); h->slice_has_req.assign(NS_all(h), 0); }
    for (size_t i = 0; i < n * S; i++) { h->slice_traffic[f * S + i] = t->slice_traffic[i]; h->slice_has_req[f * S + i] = t->slice_has_req[i]; }
    if (h->kp.trf_gen) { const int rc = build_poisson_tables(h, stream); if (rc != RANENV_OK) return rc; }
    return RANENV_OK;
}

int ranenv_bind_se_pool(ranenv_handle h, const float *dev_pool, int64_t n_tiles, int64_t tile_stride)
{
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    h->se_mode = RANENV_SE_STREAM;             // the sidecars describe the pool they were built from
    h->se_stats_n = 0;                         // ... and so do the tile statistics
    h->ml_valid = false; h->ml_failed = false; // ... and the member-lines copy (rebuilt by the next rollout that would use it)
    if (dev_pool == nullptr) {
        h->kp.se_pool = nullptr; h->kp.se_stride = 0; h->se_tiles_n = 0; h->kp.se_quad = 0;
        return RANENV_OK;
    }
    if (n_tiles < 1 || tile_stride < (int64_t)h->cfg.n_ues * h->cfg.n_rbs)
        return fail(h, RANENV_E_INVALID, "SE pool needs n_tiles >= 1 and tile_stride >= U*R");
    h->kp.se_pool = dev_pool; h->kp.se_stride = tile_stride; h->se_tiles_n = n_tiles; h->kp.se_quad = 0;
    h->have_episodes = false;  // descriptors are re-validated against the new pool
    return RANENV_OK;
}

int ranenv_bind_se_pool_quad(ranenv_handle h, const float *dev_pool, int64_t n_tiles, int64_t tile_stride)
{
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    const int64_t need = (int64_t)((h->cfg.n_rbs + 3) / 4) * h->cfg.n_ues * 4;
    if (dev_pool == nullptr) return ranenv_bind_se_pool(h, nullptr, 0, 0);
    if (n_tiles < 1 || tile_stride < need || (tile_stride & 3) != 0 || ((uintptr_t)dev_pool & 15) != 0)
        return fail(h, RANENV_E_INVALID, "RB-quad-major SE pool needs n_tiles >= 1, tile_stride >= ceil(R/4)*U*4 = %lld floats and a multiple of 4, "
                    "and a 16-byte aligned pool", (long long)need);
    h->se_mode = RANENV_SE_STREAM; h->se_stats_n = 0;
    h->ml_valid = false; h->ml_failed = false;
    h->kp.se_pool = dev_pool; h->kp.se_stride = tile_stride; h->se_tiles_n = n_tiles; h->kp.se_quad = 1;
    h->have_episodes = false;
    return RANENV_OK;
}

int ranenv_se_retile_quad(const float *dev_rb_major, float *dev_quad, int64_t n_tiles, int32_t n_ues, int32_t n_rbs, void *stream)
{
    if (!dev_rb_major || !dev_quad) return fail(nullptr, RANENV_E_INVALID, "null argument");
    if (n_tiles < 0 || n_ues < 1 || n_rbs < 1) return fail(nullptr, RANENV_E_INVALID, "bad sizes");
    if (((uintptr_t)dev_quad & 15) != 0) return fail(nullptr, RANENV_E_INVALID, "the RB-quad-major pool must be 16-byte aligned");
    const long long n_quads = (long long)n_tiles * ((n_rbs + 3) / 4) * n_ues;
    if (n_quads == 0) return RANENV_OK;
    long long blocks = (n_quads + 255) / 256;
    if (blocks > 256 * 64) blocks = 256 * 64;
    launch_se_retile_quad((hipStream_t)stream, (unsigned)blocks, dev_rb_major, dev_quad, n_quads, (int)n_ues, (int)n_rbs);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(nullptr, RANENV_E_HIP, "se_retile_quad launch: %s", hipGetErrorString(e));
    return RANENV_OK;
}

int ranenv_se_retile_member_lines(const float *dev_pool, int32_t quad, int64_t tile_stride, float *dev_lines, int64_t n_tiles, int32_t n_ues,
                                  int32_t n_rbs, void *stream)
{
    if (!dev_pool || !dev_lines) return fail(nullptr, RANENV_E_INVALID, "null argument");
    if (n_tiles < 0 || n_ues < 1 || n_rbs < 1) return fail(nullptr, RANENV_E_INVALID, "bad sizes");
    const int64_t need = quad ? (int64_t)((n_rbs + 3) / 4) * n_ues * 4 : (int64_t)n_ues * n_rbs;
    if (tile_stride < need) return fail(nullptr, RANENV_E_INVALID, "tile_stride %lld is below a tile's %lld floats", (long long)tile_stride, (long long)need);
    if (((uintptr_t)dev_lines & 15) != 0) return fail(nullptr, RANENV_E_INVALID, "the member-lines copy must be 16-byte aligned");
    MemberLineTable tb;
    if (!member_line_table((int)n_rbs, &tb)) return fail(nullptr, RANENV_E_INVALID, "n_rbs %d needs more than %d lines per UE", (int)n_rbs, (int)MEMBER_LINES_MAX);
    const long long burst = 1ll << 16;
    for (long long t0 = 0; t0 < n_tiles; t0 += burst) {
        const long long n = n_tiles - t0 < burst ? n_tiles - t0 : burst;
        long long blocks = (n * n_ues * tb.lines * 8 + 255) / 256;
        if (blocks > 256 * 64) blocks = 256 * 64;
        launch_se_retile_member_lines((hipStream_t)stream, (unsigned)blocks, dev_pool + (size_t)t0 * (size_t)tile_stride, (long long)tile_stride, quad ? 1 : 0,
                                      dev_lines + (size_t)t0 * (size_t)n_ues * tb.lines * 32, n, (int)n_ues, (int)n_rbs, tb);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(nullptr, RANENV_E_HIP, "se_retile_member_lines launch: %s", hipGetErrorString(e));
    return RANENV_OK;
}

int ranenv_member_line_plan(int32_t n_rbs, int32_t max_lines, int32_t *leaf, int32_t *first_rb, int32_t *groups)
{
    if (n_rbs < 1 || max_lines < 0) return fail(nullptr, RANENV_E_INVALID, "bad sizes");
    const std::vector<MemberLine> plan = member_line_plan((int)n_rbs);
    for (size_t l = 0; l < plan.size() && l < (size_t)max_lines; l++) {
        if (leaf) leaf[l] = plan[l].leaf;
        if (first_rb) first_rb[l] = plan[l].rb0;
        if (groups) groups[l] = plan[l].groups;
    }
    return (int)plan.size();
}

// (restates member_line_sums' serving slots, ranenv_numeric.hpp: prefix lanes keep their number, then holders, members, the rest)
int ranenv_member_serving_order(uint64_t member_mask, uint64_t holder_mask, int32_t lines_per_ue, int32_t dq, int32_t *slots, int32_t *masked_passes)
{
    if (!slots || !masked_passes) return fail(nullptr, RANENV_E_INVALID, "null argument");
    if (lines_per_ue < 1 || dq < 1 || (holder_mask & ~member_mask) != 0) return fail(nullptr, RANENV_E_INVALID, "bad sizes, or a holder that is no member");
    const int p0 = (dq + lines_per_ue - 1) / lines_per_ue;
    if (p0 > 8) return fail(nullptr, RANENV_E_INVALID, "dq %d at %d lines per UE: the prefix exceeds the wave", (int)dq, (int)lines_per_ue);
    const int pre = p0 * 8;
    int top = 0;
    for (int l = 0; l < 64; l++) if (member_mask >> l & 1) top = l + 1;
    int next = pre;
    for (int l = 0; l < pre; l++) slots[l] = l;
    for (int group = 0; group < 3; group++)          // holders, members without an RB, lanes without a member
        for (int l = pre; l < 64; l++) {
            const bool m = member_mask >> l & 1, hd = holder_mask >> l & 1;
            if ((group == 0 && hd) || (group == 1 && m && !hd) || (group == 2 && !m)) slots[l] = next++;
        }
    int holders_behind = 0;
    for (int l = pre; l < 64; l++) holders_behind += (int)(holder_mask >> l & 1);
    const int passes = (top + 7) / 8, want = p0 + (holders_behind + 7) / 8;
    *masked_passes = want < passes ? want : passes;
    return RANENV_OK;
}

int ranenv_member_lines_row_sums_host(const float *row_lines, int32_t n_rbs, int32_t rb_start, int32_t rb_count, double *full, double *part)
{
    if (!row_lines || !full || !part) return fail(nullptr, RANENV_E_INVALID, "null argument");
    if (n_rbs < 1 || rb_start < 0 || rb_count < 0) return fail(nullptr, RANENV_E_INVALID, "bad sizes");
    const float *line = row_lines;
    member_lines_pairwise(line, 0, (int)n_rbs, (unsigned)rb_start, (unsigned)rb_count, *full, *part);
    return RANENV_OK;
}

// (restates member_line_sums + member_line_finish, ranenv_numeric.hpp.  The kernels' rows have at most two levels of halves -- A, B, T --;
// this follows numpy's recursion to any depth: the left siblings along the right spine, outermost first, then the last leaf.
// `walk`: the UE's whole-group lines; `tail8`: the R mod 8 floats the owner adds -- null: they follow the walked lines, the old layout's tail line)
static int member_owner_tail_sums(const float *walk, const float *tail8, int R, unsigned s, unsigned c, double *full, double *part)
{
    const int tail = R & 7;
    // ---- the cluster's part: the whole-group lines alone
    const float *line = walk;
    std::vector<std::pair<double, double>> left;          // (f, g) of A, B, ...
    int lo = 0, n = R;
    while (n > 128) {
        int n2 = n / 2; n2 -= n2 % 8;
        double f1, g1;
        member_lines_pairwise(line, lo, n2, s, c, f1, g1);       // (a left sibling is a multiple of 8 long: no tail line in there)
        left.push_back({f1, g1});
        lo += n2; n -= n2;
    }
    double t, tg;
    member_leaf_groups(line, lo, n, s, c, t, tg);                 // T
    const int walked = (int)((line - walk) / 32);
    // ---- the owner's finish: its own `tail` floats, then the halves from the innermost outwards
    if (!tail8) tail8 = line;
    for (int k = 0; k < tail; k++) {
        const double d = (double)tail8[k];
        t += d;
        tg = std::fma(d, ((unsigned)(R - tail + k) - s) < c ? 1.0 : 0.0, tg);
    }
    for (size_t i = left.size(); i-- > 0;) { t = left[i].first + t; tg = left[i].second + tg; }
    *full = t; *part = tg;
    return walked;
}

int ranenv_member_lines_owner_tail_sums_host(const float *row_lines, int32_t n_rbs, int32_t rb_start, int32_t rb_count, double *full, double *part,
                                             int32_t *walked_lines)
{
    if (!row_lines || !full || !part || !walked_lines) return fail(nullptr, RANENV_E_INVALID, "null argument");
    if (n_rbs < 1 || rb_start < 0 || rb_count < 0) return fail(nullptr, RANENV_E_INVALID, "bad sizes");
    *walked_lines = (int32_t)member_owner_tail_sums(row_lines, nullptr, (int)n_rbs, (unsigned)rb_start, (unsigned)rb_count, full, part);
    return RANENV_OK;
}

int ranenv_member_lines_packed_layout(int32_t n_ues, int32_t n_rbs, int32_t *walked_lines, int64_t *block_offset, int64_t *tile_bytes)
{
    if (!walked_lines || !block_offset || !tile_bytes) return fail(nullptr, RANENV_E_INVALID, "null argument");
    if (n_ues < 1 || n_rbs < 1) return fail(nullptr, RANENV_E_INVALID, "bad sizes");
    PackedLayout pk; MemberLineTable tb;
    if (!member_lines_packed_layout((int)n_ues, (int)n_rbs, &pk, &tb))
        return fail(nullptr, RANENV_E_INVALID, "n_rbs %d needs more than %d lines per UE", (int)n_rbs, (int)MEMBER_LINES_MAX);
    *walked_lines = pk.nlw; *block_offset = pk.block_off; *tile_bytes = pk.tile_bytes;
    return RANENV_OK;
}

int ranenv_se_retile_member_lines_packed(const float *dev_pool, int32_t quad, int64_t tile_stride, float *dev_lines, int64_t n_tiles, int32_t n_ues,
                                         int32_t n_rbs, void *stream)
{
    if (!dev_pool || !dev_lines) return fail(nullptr, RANENV_E_INVALID, "null argument");
    if (n_tiles < 0 || n_ues < 1 || n_rbs < 1) return fail(nullptr, RANENV_E_INVALID, "bad sizes");
    const int64_t need = quad ? (int64_t)((n_rbs + 3) / 4) * n_ues * 4 : (int64_t)n_ues * n_rbs;
    if (tile_stride < need) return fail(nullptr, RANENV_E_INVALID, "tile_stride %lld is below a tile's %lld floats", (long long)tile_stride, (long long)need);
    if (((uintptr_t)dev_lines & 15) != 0) return fail(nullptr, RANENV_E_INVALID, "the member-lines copy must be 16-byte aligned");
    PackedLayout pk; MemberLineTable tb;
    if (!member_lines_packed_layout((int)n_ues, (int)n_rbs, &pk, &tb))
        return fail(nullptr, RANENV_E_INVALID, "n_rbs %d needs more than %d lines per UE", (int)n_rbs, (int)MEMBER_LINES_MAX);
    retile_member_lines_packed((hipStream_t)stream, dev_pool, (long long)tile_stride, quad ? 1 : 0, dev_lines, (long long)n_tiles, (int)n_ues, (int)n_rbs, tb, pk);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(nullptr, RANENV_E_HIP, "se_retile_member_lines_packed launch: %s", hipGetErrorString(e));
    return RANENV_OK;
}

int ranenv_member_lines_packed_sums_host(const float *walk_lines, const float *tail_slot, int32_t n_rbs, int32_t rb_start, int32_t rb_count, double *full,
                                         double *part)
{
    if (!full || !part) return fail(nullptr, RANENV_E_INVALID, "null argument");
    if (n_rbs < 1 || rb_start < 0 || rb_count < 0) return fail(nullptr, RANENV_E_INVALID, "bad sizes");
    if ((n_rbs >= 8 && !walk_lines) || ((n_rbs & 7) != 0 && !tail_slot)) return fail(nullptr, RANENV_E_INVALID, "null argument");
    static const float none[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    (void)member_owner_tail_sums(walk_lines, tail_slot ? tail_slot : none, (int)n_rbs, (unsigned)rb_start, (unsigned)rb_count, full, part);
    return RANENV_OK;
}

int ranenv_bind_traffic_pool(ranenv_handle h, const int32_t *dev_pool, int64_t n_rows)
{
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    if (dev_pool != nullptr && n_rows < 1) return fail(h, RANENV_E_INVALID, "traffic pool needs n_rows >= 1");
    h->kp.trf_pool = dev_pool; h->trf_rows_n = dev_pool ? n_rows : 0;
    h->have_episodes = false; h->idle_check_dirty = true;
    return RANENV_OK;
}

static int check_episode(ranenv_handle h, const ranenv_episode &e, const char *what, long long idx)
{
    if (e.scenario < 0 || e.scenario >= h->cfg.n_scenarios) return fail(h, RANENV_E_INVALID, "%s %lld: scenario %d outside pool of %d", what, idx, e.scenario, h->cfg.n_scenarios);
    if (e.se_len < 1 || e.se_offset < 0 || e.se_offset >= e.se_len || e.se_base < 0 || e.trf_len < 1 ||
        e.trf_offset < 0 || e.trf_offset >= e.trf_len || e.trf_base < 0)
        return fail(h, RANENV_E_INVALID, "%s %lld: need len >= 1, 0 <= offset < len, base >= 0", what, idx);
    if (h->se_tiles_n > 0 && e.se_base + e.se_len > h->se_tiles_n)
        return fail(h, RANENV_E_INVALID, "%s %lld: SE trace [%lld,+%d) exceeds the bound pool of %lld tiles", what, idx, (long long)e.se_base, e.se_len, (long long)h->se_tiles_n);
    if (h->kp.trf_pool && e.trf_base + e.trf_len > h->trf_rows_n)
        return fail(h, RANENV_E_INVALID, "%s %lld: traffic trace [%lld,+%d) exceeds the bound pool of %lld rows", what, idx, (long long)e.trf_base, e.trf_len, (long long)h->trf_rows_n);
    return RANENV_OK;
}

int ranenv_set_episodes(ranenv_handle h, const ranenv_episode *eps, void *stream_)
{
    if (!h || !eps) return fail(h, RANENV_E_INVALID, "null argument");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    for (int b = 0; b < h->cfg.batch; b++) { const int rc = check_episode(h, eps[b], "env", b); if (rc != RANENV_OK) return rc; }
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(h, hipMemcpyAsync(h->d_episodes, eps, sizeof(ranenv_episode) * (size_t)h->cfg.batch, hipMemcpyHostToDevice, stream));
    HIP_TRY(h, hipStreamSynchronize(stream));
    h->have_episodes = true; h->idle_check_dirty = true; h->pclass_dirty = true;
    return RANENV_OK;
}

int ranenv_set_policy(ranenv_handle h, int32_t policy, int32_t fixed_intra)
{
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    if (policy < RANENV_POLICY_EXTERNAL || policy > RANENV_POLICY_HEAD_NETWORK) return fail(h, RANENV_E_INVALID, "unknown policy %d", policy);
    if (!(fixed_intra == RANENV_INTRA_RR || fixed_intra == RANENV_INTRA_PF || fixed_intra == RANENV_INTRA_MT || fixed_intra == RANENV_INTRA_PER_SLICE))
        return fail(h, RANENV_E_INVALID, "unknown intra-slice scheduler %d", fixed_intra);
    h->kp.policy = policy; h->kp.fixed_intra = fixed_intra;
    return RANENV_OK;
}

// ---- policy networks (RANENV_POLICY_NETWORK) --------------------------------------------------------------------------------
// Validate one ranenv_mlp against the handle's sizes and lay it out in the packed buffer from float `off` on (widths padded to 32).
static const struct { const char *who; bool intra; int out_s, out_1; } NET_ROLES[] = {      // intra: the input is a slice's row, else the (head)
    {"inter", false, 2, 0}, {"intra", true, 0, 3}, {"inter value", false, 0, 1}, {"intra value", true, 0, 1},      // observation [10*S];
    {"head", false, 1, 0}, {"head", false, 2, 0}, {"head value", false, 0, 1},                                     // output width out_s * S + out_1
    {"SAC critic", false, 0, 1}};                                                                                  // (input: [observation | action], 11*S)

// THE SIZE RULE of a packed copy (ranenv_packed_net_floats exposes it): the L layers of widths dims[0..L] from float `off` on, every
// width padded to 32, a bf16 net's weights two per float; returns the float behind the last bias
static long long net_pack(const int32_t *dims, int L, int prec, PolicyNet &net, long long off)
{
    const int per_float = prec == RANENV_NET_BF16 ? 2 : 1;      // weights per float of the packed copy
    for (int l = 0; l < L; l++) {
        net.kp[l] = (dims[l] + 31) / 32 * 32; net.np[l] = (dims[l + 1] + 31) / 32 * 32;
        net.w_off[l] = off; off += (long long)net.kp[l] * net.np[l] / per_float;
        net.b_off[l] = off; off += net.np[l];
    }
    return off;
}

// Floats of one packed copy of `net` (every copy is laid out from float 0 of its extent)
static long long net_floats(const PolicyNet &net) { return net.b_off[net.n_layers - 1] + net.np[net.n_layers - 1]; }

// Floats a slot's copy counts with: a mixed population's with the extent of every member, the largest member's
static long long slot_copy_floats(const ranenv::NetSlot &slot) { return slot.mixed ? slot.member_stride : net_floats(slot.net); }

// An IBSched role number as the ABI takes it
static int role_check(ranenv_handle h, int32_t role)
{
    return role >= NET_INTER && role <= NET_INTRA_VALUE ? RANENV_OK : fail(h, RANENV_E_INVALID, "role %d (0 inter actor, 1 intra actor, 2 inter critic, 3 intra critic)", role);
}

static int net_layout(ranenv_handle h, const ranenv_mlp *m, NetRole role, PolicyNet &net, long long &off)
{
    const int S = h->cfg.n_slices, Us = h->cfg.max_ues_slice;
    const char *who = NET_ROLES[role].who;
    const bool intra = NET_ROLES[role].intra;
    if (m->n_hidden < 1 || m->n_hidden > NET_MAX_LAYERS - 1) return fail(h, RANENV_E_INVALID, "%s net: %d hidden layers (1..%d)", who, m->n_hidden, NET_MAX_LAYERS - 1);
    if (m->activation != RANENV_ACT_TANH && m->activation != RANENV_ACT_RELU) return fail(h, RANENV_E_INVALID, "%s net: unknown activation %d", who, m->activation);
    if (m->precision != RANENV_NET_F32 && m->precision != RANENV_NET_BF16) return fail(h, RANENV_E_INVALID, "%s net: unknown precision %d", who, m->precision);
    if (role == NET_SAC_Q && m->precision != RANENV_NET_F32) return fail(h, RANENV_E_INVALID, "SAC critic: precision %d (the training targets stay RANENV_NET_F32)", m->precision);
    int in_dim = role == NET_SAC_Q ? 11 * S : 10 * S;
    if (!intra && m->input_layout != RANENV_NET_IN_OBS) return fail(h, RANENV_E_INVALID, "%s net: input layout %d (only RANENV_NET_IN_OBS)", who, m->input_layout);
    if (intra) {
        if (m->input_layout == RANENV_NET_IN_OBS) in_dim = 2 * Us + 9;
        else if (m->input_layout == RANENV_NET_IN_MASK_OBS) in_dim = 3 * Us + 9;
        else return fail(h, RANENV_E_INVALID, "intra net: unknown input layout %d", m->input_layout);
    }
    const int out_dim = NET_ROLES[role].out_s * S + NET_ROLES[role].out_1, L = m->n_hidden + 1;
    if (m->dims[0] != in_dim) return fail(h, RANENV_E_INVALID, "%s net: input width %d, the observation has %d", who, m->dims[0], in_dim);
    for (int i = 1; i < L; i++)
        if (m->dims[i] < 1 || m->dims[i] > NET_MAX_WIDTH) return fail(h, RANENV_E_INVALID, "%s net: hidden width %d (1..%d)", who, m->dims[i], NET_MAX_WIDTH);
    if (m->dims[L] != out_dim) return fail(h, RANENV_E_INVALID, "%s net: output width %d, expected %d", who, m->dims[L], out_dim);
    for (int i = 0; i < L; i++)
        if (!m->weight[i] || !m->bias[i]) return fail(h, RANENV_E_INVALID, "%s net: layer %d has no weight / bias", who, i);
    net = PolicyNet{};
    net.n_layers = L; net.act = m->activation; net.layout = m->input_layout; net.prec = m->precision; net.in_dim = in_dim; net.out_dim = out_dim;
    off = net_pack(m->dims, L, net.prec, net, off);
    return RANENV_OK;
}

static int net_copy(ranenv_handle h, const ranenv_mlp *m, const PolicyNet &net, hipStream_t s, float *dst)
{
    for (int l = 0; l < net.n_layers; l++) {
        const int K = m->dims[l], N = m->dims[l + 1];
        if (net.prec == RANENV_NET_BF16) launch_pack_bf16(s, m->weight[l], N, K, net.np[l], net.kp[l], (unsigned short *)(dst + net.w_off[l]));
        else HIP_TRY(h, hipMemcpy2DAsync(dst + net.w_off[l], sizeof(float) * net.kp[l], m->weight[l], sizeof(float) * K, sizeof(float) * K, N,
                                    hipMemcpyDeviceToDevice, s));
        HIP_TRY(h, hipMemcpyAsync(dst + net.b_off[l], m->bias[l], sizeof(float) * N, hipMemcpyDeviceToDevice, s));
    }
    if (net.prec == RANENV_NET_BF16) HIP_TRY(h, hipGetLastError());
    return RANENV_OK;
}

// Binding has two phases, and every ranenv_set_*_network call goes through them in one order: net_plan for all of its nets and its own
// argument checks -- an error so far precedes every HIP call and leaves every slot as it was --, hipSetDevice, its own allocations,
// net_commit for all of its nets, and last bind_flags: which forms of the IBSched roles are on now (BIND_RULES).
// THE SHAPE RULE of a slot's copies: net `a` of unpadded widths `da` beside copy 0 (or the bound set's net 0) `b` -- equal in shape,
// activation, input layout and precision; mixed (the members of a mixed population): in input layout and precision only
static bool net_agrees(bool mixed, const PolicyNet &a, const int32_t *da, const PolicyNet &b, const int32_t *db)
{
    bool same = a.layout == b.layout && a.prec == b.prec;
    if (mixed) return same;
    same = same && a.n_layers == b.n_layers && a.act == b.act;
    for (int l = 0; same && l <= a.n_layers; l++) same = da[l] == db[l];
    return same;
}

// PLAN: `copies` nets of one role (one, one per slice, or one per member: the slot's form) validated and laid out: net_layout's checks
// for every copy, each from float 0 of its extent, and the shape rule.  No HIP call, nothing of the handle changes.
struct NetBind {
    ranenv::NetSlot *slot; const ranenv_mlp *const *nets; int copies; NetRole role;
    bool mixed = false;                   // (a population's) the copies may differ in hidden widths, depth and activation
    std::vector<PolicyNet> member;        // the plan: copy i's layout (per slice: with the copies' stride) ...
    long long stride, floats;             // ... floats between two copies -- the largest copy's packed size --, floats of all copies
};
static int net_plan(ranenv_handle h, NetBind *binds, int n)
{
    for (NetBind *b = binds; b < binds + n; b++) {
        const char *who = NET_ROLES[b->role].who, *per = b->slot->form == FORM_MEMBER ? "member" : "slice";
        b->member.assign((size_t)b->copies, PolicyNet{});
        b->stride = 0;
        for (int i = 0; i < b->copies; i++) {
            const ranenv_mlp *m = b->nets[i];
            if (!m) return fail(h, RANENV_E_INVALID, "%s nets per %s: net %d is null", who, per, i);
            long long mine = 0;
            if (const int rc = net_layout(h, m, b->role, b->member[(size_t)i], mine); rc != RANENV_OK) return rc;
            if (!net_agrees(b->mixed, b->member[(size_t)i], m->dims, b->member[0], b->nets[0]->dims))
                return b->mixed ? fail(h, RANENV_E_INVALID, "%s nets per member (mixed): net %d differs from net 0 in input layout or precision", who, i)
                                : fail(h, RANENV_E_INVALID, "%s nets per %s: net %d differs from net 0 in shape, activation, input layout or precision", who, per, i);
            b->stride = mine > b->stride ? mine : b->stride;
        }
        if (b->slot->form == FORM_SLICE && b->copies > 1) b->member[0].slice_stride = b->stride;      // (the entry the slot keeps)
        b->floats = b->stride * b->copies;
    }
    return RANENV_OK;
}

// The roles' descriptor tables, allocated (zeroed) once
static int pop_tables(ranenv_handle h) { return h->d_pop_tab ? RANENV_OK : dev_alloc(h, &h->d_pop_tab, (size_t)5 * POP_MAX); }

// ranenv_set_population_policy / _value: up to two roles' member copies (the intra array may be null) planned; the count against the grouping
static int pop_plan(ranenv_handle h, int32_t n, NetBind *b, int n_binds, bool mixed)
{
    if (h->pop.n == 0) return fail(h, RANENV_E_STATE, "no population set (ranenv_set_population)");
    if (n != h->pop.n) return fail(h, RANENV_E_INVALID, "%d nets given, the population has %d members", n, h->pop.n);
    for (int i = 0; i < n_binds; i++) b[i].mixed = mixed;
    return net_plan(h, b, n_binds);
}

// While a mixed role is bound, the mixed kernels read every net of its kind through a table: a role that one net serves for all members
// gets G entries of that net.  On the caller's stream, behind every call that binds a mixed role or a one net beside one.
static int pop_tables_one_net(ranenv_handle h, hipStream_t s)
{
    if (!h->pop_mixed()) return RANENV_OK;
    for (int r = 0; r < 4; r++)
        if (const ranenv::NetSlot *t = h->tabled(r); t && t->form == FORM_ONE) launch_net_table(s, h->d_pop_tab + r * POP_MAX, 0, h->pop.n, t->net, 0);
    HIP_TRY(h, hipGetLastError());
    return RANENV_OK;
}

// COMMIT, on the caller's stream without a host sync: every slot's buffer grown -- the outgrown one stays allocated, the launches of
// earlier calls may still read it -- or zeroed over the new nets' extent; then every copy's layers; then the slots change, all or none.
static int ppo_rebound(ranenv_handle h, ranenv::NetSlot *slot, int member, hipStream_t s);

static int net_commit(ranenv_handle h, NetBind *binds, int n, hipStream_t s)
{
    for (NetBind *b = binds; b < binds + n; b++) {
        ranenv::NetSlot &slot = *b->slot;
        if (b->floats > slot.cap) {
            if (const int rc = dev_alloc(h, &slot.w, (size_t)b->floats); rc != RANENV_OK) return rc;
            slot.cap = b->floats;
        } else {
            HIP_TRY(h, hipMemsetAsync(slot.w, 0, sizeof(float) * (size_t)b->floats, s));
        }
        for (int i = 0; i < b->copies; i++) b->member[(size_t)i].w = slot.w + (size_t)i * (size_t)b->stride;
    }
    for (NetBind *b = binds; b < binds + n; b++)
        for (int i = 0; i < b->copies; i++)
            if (const int rc = net_copy(h, b->nets[i], b->member[(size_t)i], s, b->slot->w + (size_t)i * (size_t)b->stride); rc != RANENV_OK) return rc;
    for (NetBind *b = binds; b < binds + n; b++) {      // a population's role: its table -- entry i = copy i's layout at copy i's address
        if (b->slot->form != FORM_MEMBER) continue;
        PolicyNet *tab = h->d_pop_tab + b->slot->role * POP_MAX;
        if (!b->mixed) launch_net_table(s, tab, 0, b->copies, b->member[0], b->stride);
        else for (int i = 0; i < b->copies; i++) launch_net_table(s, tab, i, 1, b->member[(size_t)i], 0);
        HIP_TRY(h, hipGetLastError());
    }
    for (NetBind *b = binds; b < binds + n; b++) {      // (nets per slice keep slice 0's entry: its stride stands for the others)
        ranenv::NetSlot &slot = *b->slot;
        const size_t kept = slot.form == FORM_MEMBER ? (size_t)b->copies : 1;
        slot.on = true; slot.mixed = b->mixed; slot.member_stride = slot.form == FORM_MEMBER ? b->stride : 0;
        slot.member.assign(b->member.begin(), b->member.begin() + (long)kept); slot.member_dims.assign(kept, {});
        for (size_t i = 0; i < kept; i++) std::copy_n(b->nets[i]->dims, 6, slot.member_dims[i].begin());
        slot.derive();
    }
    for (NetBind *b = binds; b < binds + n; b++)
        if (const int rc = ppo_rebound(h, b->slot, -1, s); rc != RANENV_OK) return rc;
    return RANENV_OK;
}

// Under RANENV_POLICY_NETWORK a TTI without caller scores steps with the nets' actions: point kp at them.  1 = the nets must run
// in front of the TTI, 0 = not this policy / caller scores, < 0 = error.
static int net_use(ranenv_handle h, KP &kp)
{
    if (!kp.scores && h->kp.policy == RANENV_POLICY_HEAD_NETWORK) {
        if (!h->head.on) return fail(h, RANENV_E_STATE, "policy HEAD_NETWORK but no head policy network bound (ranenv_set_head_policy_network)");
        if (h->head_src == RANENV_HEAD_SRC_INTER) {
            if (!kp.obs_inter) return fail(h, RANENV_E_INVALID, "the policy network reads obs_inter: the step needs that buffer");
        } else if (!h->kp.head_obs)
            return fail(h, RANENV_E_STATE, "the head policy network reads dev_obs_head: none is bound (ranenv_bind_head_outputs)");
        kp.scores = h->d_net_scores;
        return 1;
    }
    if (kp.scores || h->kp.policy != RANENV_POLICY_NETWORK) return 0;
    if (!h->serving(NET_INTER)) return fail(h, RANENV_E_STATE, "policy NETWORK but no policy network bound (ranenv_set_policy_network)");
    if (!kp.obs_inter) return fail(h, RANENV_E_INVALID, "the policy network reads obs_inter: the step needs that buffer");
    if (h->serving_net(NET_INTRA) && !kp.obs_intra) return fail(h, RANENV_E_INVALID, "the intra-slice network reads obs_intra: the step needs that buffer");
    kp.scores = h->d_net_scores;
    if (h->serving_net(NET_INTRA)) { kp.intra = h->d_net_intra; kp.fixed_intra = RANENV_INTRA_PER_SLICE; }
    return 1;
}

static bool head_policy(ranenv_handle h) { return h->kp.policy == RANENV_POLICY_HEAD_NETWORK; }
// ... with RANENV_HEAD_SRC_INTER (IBSchedSB3): the head nets read the call's obs_inter rows, a recording takes the step's reward rows
static bool head_inter(ranenv_handle h) { return head_policy(h) && h->head_src == RANENV_HEAD_SRC_INTER; }
static int head_reward_cols(ranenv_handle h) { return h->head_src == RANENV_HEAD_SRC_INTER ? h->cfg.n_slices + 1 : 2; }

// The policy launches' inputs and outputs under the handle's policy (NETWORK, or HEAD_NETWORK: the head observation -- or, by the head
// policy source, the call's own obs_inter -- as obs_inter)
static PolicyIO net_io(ranenv_handle h, const KP &kp)
{
    const bool head = head_policy(h);
    PolicyIO io{};
    io.B = h->cfg.batch; io.S = h->cfg.n_slices; io.Us = h->cfg.max_ues_slice; io.W = 2 * io.Us + 9;
    io.env_id_base = h->kp.env_id_base;
    io.episode_no = ST_episode_no(h->kp); io.step_no = ST_step_no(h->kp);
    io.scores = h->d_net_scores;
    if (head) {
        io.dist = h->head_dist; io.stochastic = h->head_stochastic; io.seed = h->head_seed;
        io.obs_inter = head_inter(h) ? kp.obs_inter : h->kp.head_obs; io.log_std = h->head_dist == RANENV_HEAD_DIST_GAUSS_CLIP ? h->d_head_log_std : nullptr;
        return io;
    }
    io.stochastic = h->net_stochastic; io.seed = h->net_seed;
    io.obs_inter = kp.obs_inter; io.obs_intra = kp.obs_intra;
    io.mask_inter = ST_mask_inter(h->kp); io.mask_intra = ST_mask_intra(h->kp);
    io.intra = h->d_net_intra;
    return io;
}

static hipError_t net_launch(ranenv_handle h, const KP &kp, int e0, int n, hipStream_t s)
{
    const bool head = head_policy(h);
    const PolicyNets nets = head ? PolicyNets{true, &h->head.net, nullptr, nullptr, nullptr} : h->ibsched_nets(false);
    return launch_policy(s, nets, net_io(h, kp), nullptr, e0, n);
}

// The buffers the nets' actions go to and the step reads them from (IBSched nets and head nets share them: one policy acts at a time)
static int net_action_buffers(ranenv_handle h)
{
    if (h->d_net_scores) return RANENV_OK;
    const size_t BS = (size_t)h->cfg.batch * h->cfg.n_slices;
    const int rc = dev_alloc(h, &h->d_net_scores, BS);
    return rc == RANENV_OK ? dev_alloc(h, &h->d_net_intra, BS) : rc;
}

// THE EXCLUSIVITY RULES: what each binding call leaves on and off among the role table's slots, as sets of (role, form).  `on`: the
// form the call binds; `on_if_intra`: on where the call's optional intra argument is given, off where it is NULL -- the argument, NULL
// included, says what the intra net of that kind is now; `off`: forms that would stand in front of what the call binds, or whose
// partner it replaces.  Deliberately asymmetric: a plain policy bind ends the population altogether (its critics too; the grouping
// stays), while a population's policy bind leaves one-net critics standing -- one critic may value every member's envs.
enum BindCall { BIND_POLICY, BIND_VALUE, BIND_INTRA_POLICY, UNBIND_INTRA_POLICY, BIND_INTRA_VALUE, UNBIND_INTRA_VALUE, BIND_POP_POLICY, BIND_POP_VALUE, UNBIND_POP };
constexpr unsigned slot_bit(int role, NetForm form) { return 1u << (role * 3 + form); }
constexpr unsigned ONE(int role) { return slot_bit(role, FORM_ONE); }
constexpr unsigned SLICE(int role) { return slot_bit(role, FORM_SLICE); }
constexpr unsigned POP(int role) { return slot_bit(role, FORM_MEMBER); }
static const struct { unsigned on, on_if_intra, off; } BIND_RULES[] = {
    /* BIND_POLICY         */ {ONE(0), ONE(1), SLICE(1) | SLICE(3) | POP(0) | POP(1) | POP(2) | POP(3)},
    /* BIND_VALUE          */ {ONE(2), ONE(3), SLICE(3) | POP(2) | POP(3)},
    /* BIND_INTRA_POLICY   */ {SLICE(1), 0, 0},                       // (refused while any population slot is on)
    /* UNBIND_INTRA_POLICY */ {0, 0, SLICE(1) | SLICE(3)},            // (the critics per slice valued the actors per slice)
    /* BIND_INTRA_VALUE    */ {SLICE(3), 0, 0},
    /* UNBIND_INTRA_VALUE  */ {0, 0, SLICE(3)},
    /* BIND_POP_POLICY     */ {POP(0), POP(1), ONE(0) | ONE(1) | SLICE(1) | SLICE(3)},
    /* BIND_POP_VALUE      */ {POP(2), POP(3), ONE(2) | ONE(3) | SLICE(3)},
    /* UNBIND_POP          */ {0, 0, POP(0) | POP(1) | POP(2) | POP(3)},
};
// The last step of a binding call, behind its net_commit: the slots' flags by the call's rule
static void bind_flags(ranenv_handle h, BindCall call, bool intra = false)
{
    const auto &rule = BIND_RULES[call];
    for (int r = 0; r < 4; r++)
        for (ranenv::NetSlot &slot : h->nets[r]) {
            const unsigned bit = slot_bit(r, slot.form);
            slot.on = (rule.on & bit) ? true : ((rule.on_if_intra & bit) ? intra : ((rule.off & bit) ? false : slot.on));
        }
}

// ranenv_set_policy_network (form FORM_ONE: n = 1) / ranenv_set_population_policy[_mixed] (FORM_MEMBER: n = G): the actors in that form
static int set_actors(ranenv_handle h, NetForm form, int32_t n, const ranenv_mlp *const *inter, const ranenv_mlp *const *intra, int32_t stochastic,
                      uint64_t seed, void *stream, bool mixed = false)
{
    const bool pop = form == FORM_MEMBER;
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    if (!inter) return fail(h, RANENV_E_INVALID, pop ? "the members' inter-slice nets are required (intra may be NULL)" : "the inter-slice net is required (intra may be NULL)");
    NetBind b[2] = {{&h->nets[NET_INTER][form], inter, n, NET_INTER}, {&h->nets[NET_INTRA][form], intra, n, NET_INTRA}};
    const int nb = intra ? 2 : 1;
    int rc = pop ? pop_plan(h, n, b, nb, mixed) : net_plan(h, b, nb);
    if (rc != RANENV_OK) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    if ((rc = net_action_buffers(h)) != RANENV_OK || (pop && (rc = pop_tables(h)) != RANENV_OK)) return rc;
    if ((rc = net_commit(h, b, nb, (hipStream_t)stream)) != RANENV_OK) return rc;
    h->net_stochastic = stochastic != 0; h->net_seed = seed;
    bind_flags(h, pop ? BIND_POP_POLICY : BIND_POLICY, intra != nullptr);
    return pop_tables_one_net(h, (hipStream_t)stream);      // (none behind BIND_POLICY: it ends every population role)
}

int ranenv_set_policy_network(ranenv_handle h, const ranenv_mlp *inter, const ranenv_mlp *intra, int32_t stochastic, uint64_t seed, void *stream)
{
    return set_actors(h, FORM_ONE, 1, inter ? &inter : nullptr, intra ? &intra : nullptr, stochastic, seed, stream);
}

// ranenv_set_intra_policy_networks / _intra_value_networks: n = S nets of one shape at equal stride in the role's per-slice slot
static int net_set_copies(ranenv_handle h, BindCall call, int32_t n, const ranenv_mlp *const *nets, NetRole role, hipStream_t s)
{
    const char *who = NET_ROLES[role].who;
    if (n != h->cfg.n_slices) return fail(h, RANENV_E_INVALID, "%s nets per slice: %d given, the handle has %d slices", who, n, h->cfg.n_slices);
    if (!nets) return fail(h, RANENV_E_INVALID, "%s nets per slice: null array", who);
    NetBind b{&h->nets[role][FORM_SLICE], nets, n, role};
    if (const int rc = net_plan(h, &b, 1); rc != RANENV_OK) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    if (const int rc = net_commit(h, &b, 1, s); rc != RANENV_OK) return rc;
    bind_flags(h, call);
    return RANENV_OK;
}

int ranenv_set_intra_policy_networks(ranenv_handle h, int32_t n, const ranenv_mlp *const *actors, void *stream)
{
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    if (n == 0 && !actors) { bind_flags(h, UNBIND_INTRA_POLICY); return RANENV_OK; }
    if (h->pop_bound()) return fail(h, RANENV_E_STATE, "intra policy nets per slice while a population's nets are bound (ranenv_set_policy_network first)");
    if (!h->nets[NET_INTER][FORM_ONE].on) return fail(h, RANENV_E_STATE, "intra policy nets per slice need a bound inter net (ranenv_set_policy_network)");
    return net_set_copies(h, BIND_INTRA_POLICY, n, actors, NET_INTRA, (hipStream_t)stream);
}

int ranenv_set_intra_value_networks(ranenv_handle h, int32_t n, const ranenv_mlp *const *critics, void *stream)
{
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    if (n == 0 && !critics) { bind_flags(h, UNBIND_INTRA_VALUE); return RANENV_OK; }
    if (h->pop_bound()) return fail(h, RANENV_E_STATE, "intra value nets per slice while a population's nets are bound (ranenv_set_policy_network first)");
    const PolicyNet *ia = h->serving_net(NET_INTRA);
    if (!ia) return fail(h, RANENV_E_INVALID, "intra value nets need a bound intra policy net (ranenv_set_policy_network / ranenv_set_intra_policy_networks)");
    if (n == h->cfg.n_slices && critics && critics[0] && critics[0]->input_layout != ia->layout)
        return fail(h, RANENV_E_INVALID, "intra value nets: input layout %d, the intra policy net has %d", critics[0]->input_layout, ia->layout);
    return net_set_copies(h, BIND_INTRA_VALUE, n, critics, NET_INTRA_VALUE, (hipStream_t)stream);
}

int ranenv_get_policy_actions(ranenv_handle h, double **dev_scores, uint8_t **dev_intra)
{
    if (!h || !dev_scores || !dev_intra) return fail(h, RANENV_E_INVALID, "null argument");
    if (!h->serving(NET_INTER) && !h->head.on) return fail(h, RANENV_E_STATE, "no policy network bound (ranenv_set_policy_network)");
    *dev_scores = h->d_net_scores; *dev_intra = (h->serving(NET_INTER) && h->serving_net(NET_INTRA)) ? h->d_net_intra : nullptr;
    return RANENV_OK;
}

// ranenv_set_value_network (form FORM_ONE: n = 1) / ranenv_set_population_value[_mixed] (FORM_MEMBER: n = G): the critics in that form
static int set_critics(ranenv_handle h, NetForm form, int32_t n, const ranenv_mlp *const *inter, const ranenv_mlp *const *intra, void *stream, bool mixed = false)
{
    const bool pop = form == FORM_MEMBER;
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    if (!inter) return fail(h, RANENV_E_INVALID, pop ? "the members' inter-slice value nets are required (intra may be NULL)" : "the inter-slice value net is required (intra may be NULL)");
    const PolicyNet *ia = h->serving_net(NET_INTRA);
    if (intra && !(h->serving(NET_INTER) && ia))
        return fail(h, RANENV_E_INVALID, pop ? "intra value nets need a bound intra policy net" : "an intra value net needs a bound intra policy net (ranenv_set_policy_network)");
    // (a population's array is read only where it has the grouping's count of entries: the plan refuses every other)
    if (intra && (!pop || (h->pop.n > 0 && n == h->pop.n)) && intra[0] && intra[0]->input_layout != ia->layout)
        return fail(h, RANENV_E_INVALID, pop ? "intra value nets: input layout %d, the intra policy net has %d" : "intra value net: input layout %d, the intra policy net has %d",
                    intra[0]->input_layout, ia->layout);
    NetBind b[2] = {{&h->nets[NET_INTER_VALUE][form], inter, n, NET_INTER_VALUE}, {&h->nets[NET_INTRA_VALUE][form], intra, n, NET_INTRA_VALUE}};
    const int nb = intra ? 2 : 1;
    if (const int rc = pop ? pop_plan(h, n, b, nb, mixed) : net_plan(h, b, nb); rc != RANENV_OK) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    if (const int rc = pop ? pop_tables(h) : RANENV_OK; rc != RANENV_OK) return rc;
    if (const int rc = net_commit(h, b, nb, (hipStream_t)stream); rc != RANENV_OK) return rc;
    bind_flags(h, pop ? BIND_POP_VALUE : BIND_VALUE, intra != nullptr);
    return pop_tables_one_net(h, (hipStream_t)stream);
}

int ranenv_set_value_network(ranenv_handle h, const ranenv_mlp *inter, const ranenv_mlp *intra, void *stream)
{
    return set_critics(h, FORM_ONE, 1, inter ? &inter : nullptr, intra ? &intra : nullptr, stream);
}

// ---- populations: one net set per env group ------------------------------------------------------------------------------------
// A grouping as the ABI takes it: 1..POP_MAX members, first[0] = 0 < first[1] < ... < first[n] (= batch where one is given)
static int pop_check(ranenv_handle h, int32_t n, const int32_t *first, int batch)
{
    if (n < 1 || n > POP_MAX) return fail(h, RANENV_E_INVALID, "a population has 1..%d members, not %d", (int)POP_MAX, n);
    if (!first) return fail(h, RANENV_E_INVALID, "null first_env table");
    if (first[0] != 0) return fail(h, RANENV_E_INVALID, "first_env[0] is %d: member 0 starts at env 0", first[0]);
    for (int m = 0; m < n; m++)
        if (first[m + 1] <= first[m]) return fail(h, RANENV_E_INVALID, "first_env is not strictly increasing at member %d (%d, %d)", m, first[m], first[m + 1]);
    if (batch >= 0 && first[n] != batch) return fail(h, RANENV_E_INVALID, "first_env[%d] is %d: the last member ends at the batch, %d", n, first[n], batch);
    return RANENV_OK;
}

int ranenv_set_population(ranenv_handle h, int32_t n_members, const int32_t *host_first_env)
{
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    if (n_members == 0 && !host_first_env) { h->pop = PopMap{}; bind_flags(h, UNBIND_POP); h->gae_on = false; return RANENV_OK; }
    if (const int rc = pop_check(h, n_members, host_first_env, h->cfg.batch); rc != RANENV_OK) return rc;
    PopMap map{};
    map.n = n_members;
    for (int m = 0; m <= n_members; m++) map.first[m] = host_first_env[m];
    if (h->pop_bound() && memcmp(&map, &h->pop, sizeof(map)) != 0)
        return fail(h, RANENV_E_STATE, "the grouping cannot change while a population's nets are bound (ranenv_set_policy_network, or n_members 0, unbinds them)");
    if (memcmp(&map, &h->pop, sizeof(map)) != 0) h->gae_on = false;      // (the pairs were another grouping's)
    h->pop = map;
    return RANENV_OK;
}

int ranenv_get_population(ranenv_handle h, int32_t *n_members, int32_t *host_first_env)
{
    if (!h || !n_members) return fail(h, RANENV_E_INVALID, "null argument");
    *n_members = h->pop.n;
    if (host_first_env && h->pop.n > 0)
        for (int m = 0; m <= h->pop.n; m++) host_first_env[m] = h->pop.first[m];
    return RANENV_OK;
}

int ranenv_population_tiles(int32_t n_members, const int32_t *first_env, int32_t e0, int32_t n_envs, int32_t rows_per_env, int32_t *out_member,
                            int32_t *out_row0, int32_t *out_rows, int32_t *n_tiles)
{
    if (!n_tiles) return fail(nullptr, RANENV_E_INVALID, "null n_tiles");
    if (const int rc = pop_check(nullptr, n_members, first_env, -1); rc != RANENV_OK) return rc;
    if (e0 < 0 || n_envs < 1 || (long long)e0 + n_envs > first_env[n_members]) return fail(nullptr, RANENV_E_INVALID, "envs [%d, %d + %d) outside the population's %d", e0, e0, n_envs, first_env[n_members]);
    if (rows_per_env < 1 || (long long)n_envs * rows_per_env > INT32_MAX) return fail(nullptr, RANENV_E_INVALID, "rows_per_env %d", rows_per_env);
    int k = 0;
    for (int m = 0; m < n_members; m++) {
        PopShare sh;
        const int tiles = pop_member_tiles(first_env, m, e0, n_envs, rows_per_env, sh);
        for (int t = 0; t < tiles; t++, k++) {
            if (out_member) out_member[k] = m;
            if (out_row0) out_row0[k] = sh.row0 + t * NET_ROWS;
            if (out_rows) out_rows[k] = sh.rows - t * NET_ROWS < NET_ROWS ? sh.rows - t * NET_ROWS : NET_ROWS;
        }
    }
    *n_tiles = k;
    return RANENV_OK;
}

int ranenv_set_population_policy(ranenv_handle h, int32_t n, const ranenv_mlp *const *inter, const ranenv_mlp *const *intra, int32_t stochastic,
                                 uint64_t seed, void *stream)
{
    return set_actors(h, FORM_MEMBER, n, inter, intra, stochastic, seed, stream, false);
}

int ranenv_set_population_policy_mixed(ranenv_handle h, int32_t n, const ranenv_mlp *const *inter, const ranenv_mlp *const *intra, int32_t stochastic,
                                       uint64_t seed, void *stream)
{
    return set_actors(h, FORM_MEMBER, n, inter, intra, stochastic, seed, stream, true);
}

int ranenv_set_population_value(ranenv_handle h, int32_t n, const ranenv_mlp *const *inter, const ranenv_mlp *const *intra, void *stream)
{
    return set_critics(h, FORM_MEMBER, n, inter, intra, stream, false);
}

int ranenv_set_population_value_mixed(ranenv_handle h, int32_t n, const ranenv_mlp *const *inter, const ranenv_mlp *const *intra, void *stream)
{
    return set_critics(h, FORM_MEMBER, n, inter, intra, stream, true);
}

int ranenv_set_population_member(ranenv_handle h, int32_t member, const ranenv_mlp *inter, const ranenv_mlp *intra, const ranenv_mlp *v_inter,
                                 const ranenv_mlp *v_intra, void *stream)
{
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    if (member < 0 || member >= h->pop.n) return fail(h, RANENV_E_INVALID, "member %d outside the population's %d", member, h->pop.n);
    const ranenv_mlp *given[4] = {inter, intra, v_inter, v_intra};      // by role number
    PolicyNet ni[4];
    for (int r = 0; r < 4; r++) {           // every check of every role in front of the first device call
        const ranenv_mlp *m = given[r];
        if (!m) continue;
        const ranenv::NetSlot &slot = h->nets[r][FORM_MEMBER];
        const char *who = NET_ROLES[r].who;
        if (!slot.on) return fail(h, RANENV_E_STATE, "%s net of member %d: the population has no %s nets bound", who, member, who);
        long long floats = 0;
        if (const int rc = net_layout(h, m, (NetRole)r, ni[r], floats); rc != RANENV_OK) return rc;
        if (!net_agrees(slot.mixed, ni[r], m->dims, slot.member[0], slot.member_dims[0].data()))
            return fail(h, RANENV_E_INVALID, "%s net of member %d differs from the bound set in %sinput layout or precision", who, member, slot.mixed ? "" : "shape, activation, ");
        if (slot.mixed && floats > slot.member_stride)      // ... and any such shape fits the member's extent
            return fail(h, RANENV_E_INVALID, "%s net of member %d: its packed copy has %lld floats, the member's extent %lld (the largest member's of the bind)",
                        who, member, floats, slot.member_stride);
    }
    // while a mixed PPO binding is on, the member's new actor / critic pair of a kind keeps to the update's LDS plan: refused here, and
    // the member's weights, moments and counter stay as they are
    for (int k = 0; h->ppo.mixed && k < 2; k++) {
        const ranenv::NetSlot &sa = h->nets[k][FORM_MEMBER], &sc = h->nets[2 + k][FORM_MEMBER];
        if (!sa.on || (!given[k] && !given[2 + k])) continue;
        const PolicyNet &a = given[k] ? ni[k] : sa.member[(size_t)member], *c = given[2 + k] ? &ni[2 + k] : (sc.on ? &sc.member[(size_t)member] : nullptr);
        if (h->ppo.wide) {        // (the wide plan in its place, and the share of the scratch the bind gave every workgroup)
            if (const size_t lds = ppo_wide_lds_bytes(a, c); lds > (size_t)PPO_LDS_MAX)
                return fail(h, RANENV_E_STATE, "member %d: its new %s nets need %zu bytes of LDS for two 32-row buffers of the wide plan, the bound PPO update has %d",
                            member, k ? "intra" : "inter", lds, (int)PPO_LDS_MAX);
            if (const long long p = ppo_wide_scratch(a, c); p > h->ppo_park_stride)
                return fail(h, RANENV_E_STATE, "member %d: its new %s nets park %lld floats of rows per workgroup, ranenv_ppo_bind_wide allocated %lld",
                            member, k ? "intra" : "inter", p, h->ppo_park_stride);
            continue;
        }
        if (const size_t lds = ppo_lds_bytes(a, c); lds > (size_t)PPO_LDS_MAX)
            return fail(h, RANENV_E_STATE, "member %d: its new %s nets need %zu bytes of LDS for their 32-row activations of all layers, the bound PPO update has %d",
                        member, k ? "intra" : "inter", lds, (int)PPO_LDS_MAX);
    }
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    for (int r = 0; r < 4; r++) {
        const ranenv_mlp *m = given[r];
        if (!m) continue;
        ranenv::NetSlot &slot = h->nets[r][FORM_MEMBER];
        float *dst = slot.w + (size_t)member * (size_t)slot.member_stride;
        if (!slot.mixed) {
            if (const int rc = net_copy(h, m, slot.net, s, dst); rc != RANENV_OK) return rc;
            if (const int rc = ppo_rebound(h, &slot, member, s); rc != RANENV_OK) return rc;
            continue;
        }
        // a mixed role: the extent zeroed, the layers at the new shape's offsets, then the member's table entry -- in that order
        HIP_TRY(h, hipMemsetAsync(dst, 0, sizeof(float) * (size_t)slot.member_stride, s));
        ni[r].w = dst;
        if (const int rc = net_copy(h, m, ni[r], s, dst); rc != RANENV_OK) return rc;
        launch_net_table(s, h->d_pop_tab + r * POP_MAX, member, 1, ni[r], 0);
        HIP_TRY(h, hipGetLastError());
        slot.member[(size_t)member] = ni[r];
        for (int l = 0; l < 6; l++) slot.member_dims[(size_t)member][(size_t)l] = m->dims[l];
        slot.derive();
        if (const int rc = ppo_rebound(h, &slot, member, s); rc != RANENV_OK) return rc;
    }
    return RANENV_OK;
}

int ranenv_get_population_net(ranenv_handle h, int32_t role, int32_t member, int32_t *n_hidden, int32_t *dims, int32_t *activation, int64_t *extent_floats,
                              int64_t *used_floats)
{
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    if (const int rc = role_check(h, role); rc != RANENV_OK) return rc;
    if (member < 0 || member >= h->pop.n) return fail(h, RANENV_E_INVALID, "member %d outside the population's %d", member, h->pop.n);
    const ranenv::NetSlot &slot = h->nets[role][FORM_MEMBER];      // (on: it serves the role)
    if (!slot.on) return fail(h, RANENV_E_STATE, "the population has no net of role %d bound", role);
    const PolicyNet &net = slot.member[(size_t)member];
    if (n_hidden) *n_hidden = net.n_layers - 1;
    if (dims) for (int l = 0; l < 6; l++) dims[l] = l <= net.n_layers ? slot.member_dims[(size_t)member][(size_t)l] : 0;
    if (activation) *activation = net.act;
    if (extent_floats) *extent_floats = slot.member_stride;
    if (used_floats) *used_floats = net_floats(net);
    return RANENV_OK;
}

int ranenv_packed_net_floats(int32_t n_hidden, const int32_t *dims, int32_t precision, int64_t *floats)
{
    if (!dims || !floats) return fail(nullptr, RANENV_E_INVALID, "null argument");
    if (n_hidden < 1 || n_hidden > NET_MAX_LAYERS - 1) return fail(nullptr, RANENV_E_INVALID, "%d hidden layers (1..%d)", n_hidden, NET_MAX_LAYERS - 1);
    if (precision != RANENV_NET_F32 && precision != RANENV_NET_BF16) return fail(nullptr, RANENV_E_INVALID, "unknown precision %d", precision);
    if (dims[0] < 1 || dims[n_hidden + 1] < 1) return fail(nullptr, RANENV_E_INVALID, "input width %d, output width %d", dims[0], dims[n_hidden + 1]);
    for (int l = 1; l <= n_hidden; l++)
        if (dims[l] < 1 || dims[l] > NET_MAX_WIDTH) return fail(nullptr, RANENV_E_INVALID, "hidden width %d (1..%d)", dims[l], NET_MAX_WIDTH);
    PolicyNet net{};
    *floats = net_pack(dims, n_hidden + 1, precision, net, 0);
    return RANENV_OK;
}

// ranenv_set_population_gae / ranenv_gae_population: n pairs for the population's n members
static int gae_pairs_check(ranenv_handle h, int32_t n, const double *gamma, const double *lambda)
{
    if (h->pop.n == 0) return fail(h, RANENV_E_STATE, "no population set (ranenv_set_population)");
    if (n != h->pop.n) return fail(h, RANENV_E_INVALID, "%d (gamma, lambda) pairs given, the population has %d members", n, h->pop.n);
    if (!gamma || !lambda) return fail(h, RANENV_E_INVALID, "gamma and lambda are both required");
    return RANENV_OK;
}

int ranenv_set_population_gae(ranenv_handle h, int32_t n, const double *host_gamma, const double *host_lambda)
{
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    if (!host_gamma && !host_lambda) { h->gae_on = false; return RANENV_OK; }
    if (const int rc = gae_pairs_check(h, n, host_gamma, host_lambda); rc != RANENV_OK) return rc;
    for (int m = 0; m < n; m++) { h->gae_gamma[m] = host_gamma[m]; h->gae_lambda[m] = host_lambda[m]; }
    h->gae_on = true;
    return RANENV_OK;
}

// ---- PPO update (include/ranenv.h "PPO update"; the kernel: ranenv_ppo.hip) -----------------------------------------------------
static_assert(sizeof(ranenv_ppo_hparams) == RANENV_PPO_HPARAMS_BYTES, "ranenv_ppo_hparams: 8 doubles and 4 int32");

// Floats of `net`'s F32 packed layout whatever its precision (net_pack's rule for RANENV_NET_F32); bf non-null: its offsets there
static long long net_floats_f32(const PolicyNet &net, PpoBf16Net *bf = nullptr)
{
    long long off = 0;
    for (int l = 0; l < net.n_layers; l++) {
        if (bf) bf->w_off[l] = off;
        off += (long long)net.kp[l] * net.np[l];
        if (bf) bf->b_off[l] = off;
        off += net.np[l];
    }
    return off;
}

// Member m's nets of kind k among the slots the update trains (ppo_roles): the packed floats of its actor and critic (0: none) and
// the LDS bytes their update needs -- `wide`: under the wide plan, and `park`, the floats of scratch its workgroup parks its rows in.
// A uniform binding's members all have copy 0's shape.  bf16 (ranenv_ppo_bind_spread_bfloat): the floats of the nets' F32 packed layout
// -- the masters', moments', slabs' and gradient's -- and the LDS bytes of the bf16 plan.
static void ppo_member_shape(ranenv::NetSlot *const (&slot)[4], bool mixed, int m, int k, long long &actor_floats, long long &critic_floats, size_t &lds,
                             bool wide = false, long long *park = nullptr, bool bf16 = false)
{
    const size_t i = mixed ? (size_t)m : 0;
    const PolicyNet &a = slot[k]->member[i], *c = slot[2 + k] ? &slot[2 + k]->member[i] : nullptr;
    if (bf16) { actor_floats = net_floats_f32(a); critic_floats = c ? net_floats_f32(*c) : 0; lds = ppo_bf16_lds_bytes(a, c); }
    else { actor_floats = net_floats(a); critic_floats = c ? net_floats(*c) : 0; lds = wide ? ppo_wide_lds_bytes(a, c) : ppo_lds_bytes(a, c); }
    if (park) *park = wide ? ppo_wide_scratch(a, c) : 0;
}

// THE walk over the shapes the update trains: f(member, kind, actor + critic floats, LDS bytes, parked floats) for every bound kind
// and (a mixed binding) every one of the `members`, in order, until one returns other than RANENV_OK
static int ppo_each_shape(ranenv::NetSlot *const (&slot)[4], bool mixed, bool wide, int members, const std::function<int(int, int, long long, size_t, long long)> &f,
                          bool bf16 = false)
{
    for (int k = 0; k < 2; k++) {
        if (!slot[k]) continue;
        for (int m = 0; m < (mixed ? members : 1); m++) {
            long long af, cf, park; size_t lds;
            ppo_member_shape(slot, mixed, m, k, af, cf, lds, wide, &park, bf16);
            if (const int rc = f(m, k, af + cf, lds, park); rc != RANENV_OK) return rc;
        }
    }
    return RANENV_OK;
}

// The largest needs over that walk: the gradient's floats, the LDS bytes -- of kinds < lds_kinds alone: a call that updates no intra
// rows launches with the inter nets' -- and (wide) the parked floats per workgroup
struct PpoPlan { long long grad_floats; size_t lds; long long park; };
static PpoPlan ppo_plan(ranenv::NetSlot *const (&slot)[4], bool mixed, bool wide, int members, int lds_kinds = 2, bool bf16 = false)
{
    PpoPlan p{};
    ppo_each_shape(slot, mixed, wide, members, [&](int, int k, long long floats, size_t lds, long long park) {
        p.grad_floats = std::max(p.grad_floats, floats);
        if (k < lds_kinds) p.lds = std::max(p.lds, lds);
        p.park = std::max(p.park, park);
        return (int)RANENV_OK;
    }, bf16);
    return p;
}

// `slot`'s Adam moments and gradient scratch (3 x cap floats; an outgrown allocation grows, a larger one stays, like the weights'), zeroed
static int opt_ensure(ranenv_handle h, ranenv::NetSlot *slot, hipStream_t s)
{
    if (slot->opt_cap < slot->cap) {
        if (const int rc = dev_alloc(h, &slot->opt, 3 * (size_t)slot->cap); rc != RANENV_OK) return rc;
        slot->opt_cap = slot->cap;
    }
    HIP_TRY(h, hipMemsetAsync(slot->opt, 0, sizeof(float) * 3 * (size_t)slot->opt_cap, s));
    return RANENV_OK;
}

// The slots the update trains, by role number -- the serving ones (null: none bound) -- and the member count, or what the bind of that
// geometry refuses: ranenv_ppo_bind (mixed: ranenv_ppo_bind_mixed, whose LDS plan holds per member; wide: ranenv_ppo_bind_wide, which
// checks the wide plan in its place; spread: ranenv_ppo_bind_spread, which takes one member alone), or (slices) ranenv_ppo_bind_slices -- the one-net inter pair, the intra actors per slice, the
// intra critics per slice or none.  The two geometries differ in the forms they take, the two rule blocks; their place around the
// inter pair's check is the order in which a caller who breaks two rules hears of them.  No device call.
// bf16 (ranenv_ppo_bind_spread_bfloat, a spread binding): every bound role a RANENV_NET_BF16 one-net slot, the pairs within the bf16 LDS plan.
static int ppo_roles(ranenv_handle h, bool slices, ranenv::NetSlot *(&slot)[4], int &members, bool mixed = false, bool wide = false, bool spread = false,
                     bool bf16 = false)
{
    if (h->kp.policy == RANENV_POLICY_HEAD_NETWORK) return fail(h, RANENV_E_STATE, "the PPO update trains the IBSched nets: the policy is RANENV_POLICY_HEAD_NETWORK");
    int n_pop = 0, n_one = 0;
    for (int r = 0; r < 4; r++) {
        slot[r] = h->serving(r);
        if (!slot[r]) continue;
        if (bf16 && slot[r]->form != FORM_ONE)
            return fail(h, RANENV_E_STATE, "the bf16 spread PPO update trains one agent's single nets, no population and no nets per slice: the %s nets are bound per %s",
                        NET_ROLES[r].who, slot[r]->form == FORM_MEMBER ? "member" : "slice");
        if (slices && slot[r]->form == FORM_MEMBER) return fail(h, RANENV_E_STATE, "the per-slice PPO update trains no population: the %s nets are bound per member", NET_ROLES[r].who);
        if (!slices && slot[r]->form == FORM_SLICE) return fail(h, RANENV_E_STATE, "the PPO update does not train intra nets per slice (non-shared intra policies)");
        (slot[r]->form == FORM_MEMBER ? n_pop : n_one) += 1;
    }
    if (!slices && h->pop_mixed() && !mixed) return fail(h, RANENV_E_STATE, "ranenv_ppo_bind does not train a mixed population: use ranenv_ppo_bind_mixed");
    if (!slices && mixed && !h->pop_mixed()) return fail(h, RANENV_E_STATE, "ranenv_ppo_bind_mixed trains a mixed population and no bound role is mixed: use ranenv_ppo_bind");
    if (!slot[0] || !slot[2]) return fail(h, RANENV_E_STATE, "the PPO update needs a bound inter actor and inter critic (ranenv_set_policy_network, ranenv_set_value_network)");
    if (slices) {       // the intra nets per slice, every one
        if (!slot[1]) return fail(h, RANENV_E_STATE, "the per-slice PPO update needs intra actors per slice (ranenv_set_intra_policy_networks)");
        for (int r = 1; r < 4; r += 2)
            if (slot[r] && slot[r]->form != FORM_SLICE)
                return fail(h, RANENV_E_STATE, "the per-slice PPO update needs the %s nets per slice: a net the slices share has no one owner", NET_ROLES[r].who);
    } else if (n_pop && n_one)      // every net per member, or every net single
        return fail(h, RANENV_E_STATE, "the PPO update needs every net per member or every net single: a net the members share has no one owner");
    members = n_pop ? h->pop.n : 1;
    if (spread && members > 1) return fail(h, RANENV_E_STATE, "the spread PPO update trains no population: the nets are bound per member and the population has %d", members);
    int n_bf = 0, n_f32 = 0, first_f32 = -1;
    for (int r = 0; r < 4; r++) {
        if (!slot[r]) continue;
        if (slot[r]->net.prec != RANENV_NET_F32) {
            if (!bf16) return fail(h, RANENV_E_STATE, "the PPO update trains float32 nets: the %s net is bf16", NET_ROLES[r].who);
            n_bf++;
        } else if (n_f32++ == 0) first_f32 = r;
    }
    if (bf16 && n_bf == 0) return fail(h, RANENV_E_STATE, "ranenv_ppo_bind_spread_bfloat trains RANENV_NET_BF16 nets: the bound nets are float32 (ranenv_ppo_bind_spread trains those)");
    if (bf16 && n_f32) return fail(h, RANENV_E_STATE, "ranenv_ppo_bind_spread_bfloat trains nets of one precision: the %s net is float32 beside bf16 nets", NET_ROLES[first_f32].who);
    return ppo_each_shape(slot, mixed, wide, members, [&](int m, int k, long long, size_t lds, long long) {
        if (lds <= (size_t)PPO_LDS_MAX) return (int)RANENV_OK;
        char whose[40];      // (a member binding under either of its plans names the member)
        if (!slices && !spread && (mixed || wide)) snprintf(whose, sizeof(whose), "member %d: its %s nets", m, k ? "intra" : "inter");
        else snprintf(whose, sizeof(whose), "the %s nets", k ? "intra" : "inter");
        return fail(h, RANENV_E_STATE, "%s need %zu bytes of LDS for %s, the update has %d", whose, lds,
                    bf16 ? "their 32-row bf16 activations of all layers" : (wide ? "two 32-row buffers of the wide plan" : "their 32-row activations of all layers"),
                    (int)PPO_LDS_MAX);
    }, bf16);
}

// A mixed binding's per-member packed floats [4][POP_MAX] (0: the role is not bound) as the slots stand, to the device on the caller's stream
static int ppo_floats_upload(ranenv_handle h, hipStream_t s)
{
    auto &f = h->ppo_floats;
    memset(f, 0, sizeof(f));
    for (int r = 0; r < 4; r++) {
        const ranenv::NetSlot &slot = h->nets[r][FORM_MEMBER];
        if (!slot.on) continue;
        for (size_t m = 0; m < slot.member.size() && m < (size_t)POP_MAX; m++) f[r][m] = net_floats(slot.member[m]);
    }
    HIP_TRY(h, hipMemcpyAsync(h->d_ppo_floats, f, sizeof(f), hipMemcpyHostToDevice, s));
    return RANENV_OK;
}

// A binding call has replaced `slot`'s nets (member < 0: all of them): their moments and their units' step counters start again, on
// the caller's stream -- or, where the slot has no moments of its size, the PPO binding ends.  Under ranenv_ppo_bind_slices the inter
// pair lives in the one-net slots and the intra pairs in the per-slice slots: a re-bound net of another form takes the nets out of
// that form, which ends the binding too, and a per-slice bind replaces all S copies -- their moments and the S slice counters restart.
static int ppo_head_rebound(ranenv_handle h, ranenv::NetSlot *slot, hipStream_t s);
static int sac_rebound(ranenv_handle h, ranenv::NetSlot *slot, hipStream_t s);

// ranenv_ppo_bind_spread_bfloat: what the kernels take of the one-net slot `slot` beside its PpoNet -- the F32 layout's offsets, the acting
// copy and the transposed one -- and its PpoNet: the master, m, v and g in role r's buffer, ppo_bf_cap[r] floats each
static PpoBf16Net ppo_bf16_net(ranenv_handle h, const ranenv::NetSlot *slot)
{
    PpoBf16Net n{};
    if (!slot) return n;
    net_floats_f32(slot->net, &n);
    n.acting = slot->w; n.wt = h->d_ppo_bf[slot->role] + 4 * h->ppo_bf_cap[slot->role];
    return n;
}
static PpoNet ppo_bf16_state(ranenv_handle h, const ranenv::NetSlot *slot)
{
    PpoNet n{};
    if (!slot) return n;
    const long long cap = h->ppo_bf_cap[slot->role];
    n.net = slot->net; n.net.w = nullptr;
    n.w = h->d_ppo_bf[slot->role]; n.m = n.w + cap; n.v = n.w + 2 * cap; n.g = n.w + 3 * cap;
    n.floats = net_floats_f32(slot->net);
    return n;
}
static bool ppo_bf16_fits(ranenv_handle h, const ranenv::NetSlot *slot)
{
    const int r = slot->role;
    return slot->net.prec == RANENV_NET_BF16 && h->d_ppo_bf[r] && net_floats_f32(slot->net) <= h->ppo_bf_cap[r] && net_floats(slot->net) <= h->ppo_bf_cap16[r];
}
// The master and the transposed copy of `slot`'s net from its acting copy, on the caller's stream (the bind and every re-bind)
static int ppo_bf16_seed(ranenv_handle h, const ranenv::NetSlot *slot, hipStream_t s)
{
    HIP_TRY(h, launch_ppo_bf16_seed(s, slot->net, ppo_bf16_net(h, slot), h->d_ppo_bf[slot->role], net_floats_f32(slot->net)));
    return RANENV_OK;
}

static int ppo_rebound(ranenv_handle h, ranenv::NetSlot *slot, int member, hipStream_t s)
{
    if (slot == &h->head || slot == &h->sac_q1 || slot == &h->sac_q2)
        if (const int rc = sac_rebound(h, slot, s); rc != RANENV_OK) return rc;
    if (slot == &h->head || slot == &h->head_value) return ppo_head_rebound(h, slot, s);
    const ranenv::PpoBinding b = h->ppo;
    if (!b.on) return RANENV_OK;
    if (slot->role < 0) return RANENV_OK;      // (a net the update never trains)
    if (b.bf16) {       // the master re-seeded from the new acting copy, Wt rebuilt, the kind's moments and counter restarted -- or the binding ends
        if (slot->form != FORM_ONE) return RANENV_OK;      // (nets per slice or per member now serve the role: the next update refuses them in its words)
        if (!ppo_bf16_fits(h, slot)) { h->ppo = {}; return RANENV_OK; }
        if (const int rc = ppo_bf16_seed(h, slot, s); rc != RANENV_OK) return rc;
        for (const int r : {slot->role, slot->role ^ 2})
            if (h->d_ppo_bf[r]) HIP_TRY(h, hipMemsetAsync(h->d_ppo_bf[r] + h->ppo_bf_cap[r], 0, sizeof(float) * 2 * (size_t)h->ppo_bf_cap[r], s));
        HIP_TRY(h, hipMemsetAsync(h->d_ppo_t + b.wg(slot->role & 1, 0), 0, sizeof(int32_t), s));
        return RANENV_OK;
    }
    if (!b.slices && slot->form == FORM_SLICE) return RANENV_OK;      // (... nor does a member binding train the nets per slice)
    const int kind = slot->role & 1;
    if ((b.slices && slot->form != (kind ? FORM_SLICE : FORM_ONE)) || !slot->opt || slot->cap > slot->opt_cap) { h->ppo = {}; return RANENV_OK; }
    if (b.slices) member = -1;
    // (actor and critic of a kind share the step counter: the partner net -- critic of an actor, actor of a critic -- restarts with it,
    //  or its old moments would meet the bias correction of t = 1)
    ranenv::NetSlot *both[2] = {slot, &h->nets[slot->role ^ 2][slot->form]};
    for (ranenv::NetSlot *x : both) {
        if (!x->on || !x->opt || x->cap > x->opt_cap) continue;
        if (member < 0) {
            HIP_TRY(h, hipMemsetAsync(x->opt, 0, sizeof(float) * 2 * (size_t)x->opt_cap, s));
            continue;
        }
        // (a mixed binding: the member's WHOLE extent -- another shape moves every offset, and no moment of the old one may stay in the tail)
        const size_t at = (size_t)member * (size_t)x->member_stride, n = (size_t)(b.mixed ? x->member_stride : net_floats(x->net));
        HIP_TRY(h, hipMemsetAsync(x->opt + at, 0, sizeof(float) * n, s));
        HIP_TRY(h, hipMemsetAsync(x->opt + x->opt_cap + at, 0, sizeof(float) * n, s));
    }
    // the counters of the kind's units: the slices' lie side by side, the members' two apart
    if (b.slices) HIP_TRY(h, hipMemsetAsync(h->d_ppo_t + b.wg(kind, 0), 0, sizeof(int32_t) * (size_t)b.units(kind, 1, h->cfg.n_slices), s));
    else if (member < 0) HIP_TRY(h, hipMemset2DAsync(h->d_ppo_t + b.wg(kind, 0), 2 * sizeof(int32_t), 0, sizeof(int32_t), POP_MAX, s));
    else HIP_TRY(h, hipMemsetAsync(h->d_ppo_t + b.wg(kind, member), 0, sizeof(int32_t), s));
    return b.mixed ? ppo_floats_upload(h, s) : RANENV_OK;
}

// What a spread binding of these slots holds beside the moments: floats of gradient slabs and of parked rows (wide) -- per bound kind
// `slabs` times the pair's need, the kinds back to back --, and the reduce / apply blocks of the larger kind.  The doubles of one
// kind: block partials, slab statistics, running sums.
// n_slices > 0 (ranenv_ppo_bind_slices_spread): the intra kind's need once per slice, and 1 + n_slices units of doubles for the two kinds'.
struct PpoSpreadNeed { long long slab, park, blocks; int units; };
static PpoSpreadNeed ppo_spread_need(ranenv::NetSlot *const (&slot)[4], bool wide, int slabs, bool bf16 = false, int n_slices = 0)
{
    PpoSpreadNeed n{};
    n.units = n_slices > 0 ? 1 + n_slices : 2;
    ppo_each_shape(slot, false, wide, 1, [&](int, int k, long long floats, size_t, long long park) {
        const long long copies = (long long)slabs * (k == 1 && n_slices > 0 ? n_slices : 1);
        n.slab += floats * copies; n.park += park * copies;
        n.blocks = std::max(n.blocks, (floats + PPO_SPREAD_BLOCK - 1) / PPO_SPREAD_BLOCK);
        return (int)RANENV_OK;
    }, bf16);
    return n;
}
static long long ppo_spread_doubles(long long blocks) { return blocks + PPO_SPREAD_SLABS_MAX * PPO_SPREAD_STATS + RANENV_PPO_STATS; }

// ranenv_ppo_bind / ranenv_ppo_bind_mixed / ranenv_ppo_bind_wide / ranenv_ppo_bind_slices / ranenv_ppo_bind_spread / ranenv_ppo_bind_slices_spread
static int ppo_bind(ranenv_handle h, ranenv::PpoBinding b, void *stream)
{
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    ranenv::NetSlot *slot[4];
    int members = 1;
    if (const int rc = ppo_roles(h, b.slices, slot, members, b.mixed, b.wide, b.slabs > 0, b.bf16); rc != RANENV_OK) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    if (b.slabs) {      // the spread binding's own: slabs, block partials, slab statistics and running sums, and (wide) the parked rows per slab
        const PpoSpreadNeed need = ppo_spread_need(slot, b.wide, b.slabs, b.bf16, b.slices ? h->cfg.n_slices : 0);
        if (h->ppo_slab_cap < need.slab) {
            if (const int rc = dev_alloc(h, &h->d_ppo_slab, (size_t)need.slab); rc != RANENV_OK) return rc;
            h->ppo_slab_cap = need.slab;
        }
        if (!h->d_ppo_spread || h->ppo_spread_blocks < need.blocks || h->ppo_spread_units < need.units) {      // (an outgrown one grows in both extents)
            const long long blocks = std::max(need.blocks, h->ppo_spread_blocks);
            const int units = std::max(need.units, h->ppo_spread_units);
            if (const int rc = dev_alloc(h, &h->d_ppo_spread, (size_t)units * (size_t)ppo_spread_doubles(blocks)); rc != RANENV_OK) return rc;
            h->ppo_spread_blocks = blocks; h->ppo_spread_units = units;
        }
        if (h->ppo_park_cap < need.park) {
            if (const int rc = dev_alloc(h, &h->d_ppo_park, (size_t)need.park); rc != RANENV_OK) return rc;
            h->ppo_park_cap = need.park;
        }
        HIP_TRY(h, hipMemsetAsync(h->d_ppo_slab, 0, sizeof(float) * (size_t)h->ppo_slab_cap, s));
    } else if (b.wide) {       // the parked rows: the largest need over the members and the kinds, for every workgroup
        const int wgs = b.workgroups(members, h->cfg.n_slices);
        const long long need = ppo_plan(slot, b.mixed, true, members).park * wgs;
        if (h->ppo_park_cap < need) {
            if (const int rc = dev_alloc(h, &h->d_ppo_park, (size_t)need); rc != RANENV_OK) return rc;
            h->ppo_park_cap = need;
        }
        h->ppo_park_stride = h->ppo_park_cap / wgs;                 // (a kept larger allocation serves larger re-bound shapes)
        h->ppo_park_stride -= h->ppo_park_stride % 4;               // (every workgroup's share starts on a 16-byte boundary)
    }
    if (!h->d_ppo_t) {
        if (const int rc = dev_alloc(h, &h->d_ppo_t, (size_t)POP_MAX * 2); rc != RANENV_OK) return rc;
        if (const int rc = dev_alloc(h, &h->d_ppo_hp, (size_t)POP_MAX); rc != RANENV_OK) return rc;
    }
    if (b.mixed && !h->d_ppo_floats)
        if (const int rc = dev_alloc(h, &h->d_ppo_floats, (size_t)4 * POP_MAX); rc != RANENV_OK) return rc;
    HIP_TRY(h, hipMemsetAsync(h->d_ppo_t, 0, sizeof(int32_t) * POP_MAX * 2, s));
    for (int r = 0; r < 4; r++) {
        if (!slot[r]) continue;
        if (!b.bf16) {
            if (const int rc = opt_ensure(h, slot[r], s); rc != RANENV_OK) return rc;
            continue;
        }
        // a bf16 net's f32 state (an outgrown allocation grows, a larger one stays): zeroed, then master and Wt seeded from the acting copy
        const long long f32 = net_floats_f32(slot[r]->net), f16 = net_floats(slot[r]->net);
        if (!h->d_ppo_bf[r] || h->ppo_bf_cap[r] < f32 || h->ppo_bf_cap16[r] < f16) {
            const long long c32 = std::max(f32, h->ppo_bf_cap[r]), c16 = std::max(f16, h->ppo_bf_cap16[r]);
            if (const int rc = dev_alloc(h, &h->d_ppo_bf[r], (size_t)(4 * c32 + c16)); rc != RANENV_OK) return rc;
            h->ppo_bf_cap[r] = c32; h->ppo_bf_cap16[r] = c16;
        }
        HIP_TRY(h, hipMemsetAsync(h->d_ppo_bf[r], 0, sizeof(float) * (size_t)(4 * h->ppo_bf_cap[r] + h->ppo_bf_cap16[r]), s));
        if (const int rc = ppo_bf16_seed(h, slot[r], s); rc != RANENV_OK) return rc;
    }
    h->ppo = b;
    return b.mixed ? ppo_floats_upload(h, s) : RANENV_OK;
}

int ranenv_ppo_bind(ranenv_handle h, void *stream) { return ppo_bind(h, {true, false, false, false}, stream); }
int ranenv_ppo_bind_mixed(ranenv_handle h, void *stream) { return ppo_bind(h, {true, true, false, false}, stream); }
int ranenv_ppo_bind_wide(ranenv_handle h, int32_t mixed, void *stream)
{
    if (mixed != 0 && mixed != 1) return fail(h, RANENV_E_INVALID, "mixed %d (0 as ranenv_ppo_bind, 1 as ranenv_ppo_bind_mixed)", mixed);
    return ppo_bind(h, {true, mixed == 1, true, false}, stream);
}
// (non-shared intra policies, include/ranenv.h "per slice")
int ranenv_ppo_bind_slices(ranenv_handle h, int32_t wide, void *stream)
{
    if (wide != 0 && wide != 1) return fail(h, RANENV_E_INVALID, "wide %d (0 the LDS plan, 1 the wide plan)", wide);
    return ppo_bind(h, {true, false, wide == 1, true}, stream);
}
// (one agent over the chip, include/ranenv.h "One agent over the chip")
int ranenv_ppo_bind_spread(ranenv_handle h, int32_t slabs, int32_t wide, void *stream)
{
    if (slabs < 1 || slabs > PPO_SPREAD_SLABS_MAX) return fail(h, RANENV_E_INVALID, "slabs %d (1..256)", slabs);
    if (wide != 0 && wide != 1) return fail(h, RANENV_E_INVALID, "wide %d (0 the LDS plan, 1 the wide plan)", wide);
    return ppo_bind(h, {true, false, wide == 1, false, slabs}, stream);
}
// (nets per slice over the chip, include/ranenv.h "Nets per slice over the chip")
int ranenv_ppo_bind_slices_spread(ranenv_handle h, int32_t slabs, int32_t wide, void *stream)
{
    if (slabs < 1 || slabs > PPO_SPREAD_SLABS_MAX) return fail(h, RANENV_E_INVALID, "slabs %d (1..256)", slabs);
    if (wide != 0 && wide != 1) return fail(h, RANENV_E_INVALID, "wide %d (0 the LDS plan, 1 the wide plan)", wide);
    return ppo_bind(h, {true, false, wide == 1, true, slabs}, stream);
}
// (bf16 nets over the chip, include/ranenv.h "bf16 nets over the chip")
int ranenv_ppo_bind_spread_bfloat(ranenv_handle h, int32_t slabs, void *stream)
{
    if (slabs < 1 || slabs > PPO_SPREAD_SLABS_MAX) return fail(h, RANENV_E_INVALID, "slabs %d (1..256)", slabs);
    return ppo_bind(h, {true, false, false, false, slabs, true}, stream);
}

// The bound state behind the binding of the caller's geometry (slices: ranenv_ppo_bind_slices, else one of the member bindings), or
// RANENV_E_STATE
static int ppo_bound(ranenv_handle h, bool slices, ranenv::NetSlot *(&slot)[4], int &members)
{
    const ranenv::PpoBinding &b = h->ppo;
    if (slices) {
        if (!b.on || !b.slices) return fail(h, RANENV_E_STATE, "no per-slice PPO state bound, or a binding call has outgrown it or left the per-slice form: bind again (ranenv_ppo_bind_slices)");
        for (int r = 0; r < 4; r++)
            if (const ranenv::NetSlot *x = h->serving(r); (r == 1 && !x) || (x && x->form != ((r & 1) ? FORM_SLICE : FORM_ONE)))
                return fail(h, RANENV_E_STATE, "the %s nets have left the per-slice form since ranenv_ppo_bind_slices: bind again", NET_ROLES[r].who);
    } else {
        if (!b.on) return fail(h, RANENV_E_STATE, "no PPO state bound, or a binding call has outgrown it (ranenv_ppo_bind)");
        if (b.slices) return fail(h, RANENV_E_STATE, "the PPO state was bound per slice (ranenv_ppo_bind_slices): ranenv_ppo_update_slices trains it");
    }
    if (const int rc = ppo_roles(h, slices, slot, members, b.mixed, b.wide, b.slabs > 0, b.bf16); rc != RANENV_OK) return rc;
    for (int r = 0; r < 4; r++)
        if (slot[r] && (b.bf16 ? !ppo_bf16_fits(h, slot[r]) : (!slot[r]->opt || slot[r]->opt_cap < slot[r]->cap)))
            return fail(h, RANENV_E_STATE, "the %s net was bound after %s: bind again", NET_ROLES[r].who, b.entry());
    if (b.slabs) {      // a spread binding: the slabs, block partials and parked rows of the nets as they stand fit what the bind allocated
        const PpoSpreadNeed need = ppo_spread_need(slot, b.wide, b.slabs, b.bf16, b.slices ? h->cfg.n_slices : 0);
        if (need.slab > h->ppo_slab_cap || need.blocks > h->ppo_spread_blocks || need.units > h->ppo_spread_units || need.park > h->ppo_park_cap)
            return fail(h, RANENV_E_STATE, "the bound nets need more slab or parked floats than %s allocated: bind again", b.entry());
        return RANENV_OK;
    }
    if (!b.wide) return RANENV_OK;
    // a wide binding: every workgroup's parked rows fit the share of the scratch it was given at bind
    if ((long long)b.workgroups(members, h->cfg.n_slices) * h->ppo_park_stride > h->ppo_park_cap)
        return fail(h, RANENV_E_STATE, slices ? "the parked rows were allocated for another binding: bind again" : "the population has grown since ranenv_ppo_bind_wide: bind again");
    return ppo_each_shape(slot, b.mixed, true, members, [&](int, int k, long long, size_t, long long p) {
        if (p <= h->ppo_park_stride) return (int)RANENV_OK;
        return fail(h, RANENV_E_STATE, "the %s nets park %lld floats of rows per workgroup, %s allocated %lld: bind again", k ? "intra" : "inter", p, b.entry(true), h->ppo_park_stride);
    });
}

static PpoNet ppo_net(const ranenv::NetSlot *slot)
{
    PpoNet n{};
    if (!slot) return n;
    n.net = slot->net; n.net.w = nullptr;
    n.w = slot->w; n.m = slot->opt; n.v = slot->opt + slot->opt_cap; n.g = slot->opt + 2 * slot->opt_cap;
    n.stride = slot->form == FORM_SLICE ? slot->net.slice_stride : slot->member_stride; n.floats = net_floats(slot->net);
    return n;
}

int ranenv_ppo_layout(ranenv_handle h, int64_t *grad_floats, int64_t *lds_bytes)
{
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    ranenv::NetSlot *slot[4];
    int members = 0;
    const bool mixed = h->pop_mixed(), wide = h->ppo.wide;
    if (const int rc = ppo_roles(h, h->ppo.slices, slot, members, mixed, wide, h->ppo.slabs > 0, h->ppo.bf16); rc != RANENV_OK) return rc;
    const PpoPlan plan = ppo_plan(slot, mixed, wide, members, 2, h->ppo.bf16);
    if (grad_floats) *grad_floats = plan.grad_floats;
    if (lds_bytes) *lds_bytes = (int64_t)plan.lds;
    return RANENV_OK;
}

int ranenv_ppo_member_layout(ranenv_handle h, int32_t member, int32_t kind, int64_t *actor_floats, int64_t *critic_floats, int64_t *lds_bytes)
{
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    ranenv::NetSlot *slot[4];
    int members = 0;
    const bool mixed = h->pop_mixed(), wide = h->ppo.wide;
    if (const int rc = ppo_roles(h, h->ppo.slices, slot, members, mixed, wide, h->ppo.slabs > 0, h->ppo.bf16); rc != RANENV_OK) return rc;
    members = h->ppo.units(kind, members, h->cfg.n_slices);      // (the slices' pairs have one shape: slice 0's entry answers for all)
    if (member < 0 || member >= members) return fail(h, RANENV_E_INVALID, "member %d outside the %d", member, members);
    if (kind != 0 && kind != 1) return fail(h, RANENV_E_INVALID, "kind %d (0 inter, 1 intra)", kind);
    if (!slot[kind]) return fail(h, RANENV_E_STATE, "no %s actor bound", kind ? "intra" : "inter");
    long long af, cf; size_t lds;
    ppo_member_shape(slot, mixed, member, kind, af, cf, lds, wide, nullptr, h->ppo.bf16);
    if (actor_floats) *actor_floats = af;
    if (critic_floats) *critic_floats = cf;
    if (lds_bytes) *lds_bytes = (int64_t)lds;
    return RANENV_OK;
}

// The padded layouts of an actor / critic pair given by shape alone (critic null: none): ranenv_ppo_lds_bytes / ranenv_ppo_wide_bytes
static int ppo_shape_pair(const ranenv_mlp *actor, const ranenv_mlp *critic, PolicyNet (&net)[2])
{
    const ranenv_mlp *given[2] = {actor, critic};
    for (int i = 0; i < 2; i++) {
        const ranenv_mlp *m = given[i];
        if (!m) continue;
        if (m->n_hidden < 1 || m->n_hidden > NET_MAX_LAYERS - 1) return fail(nullptr, RANENV_E_INVALID, "%d hidden layers (1..%d)", m->n_hidden, NET_MAX_LAYERS - 1);
        if (m->dims[0] < 1 || m->dims[m->n_hidden + 1] < 1) return fail(nullptr, RANENV_E_INVALID, "input width %d, output width %d", m->dims[0], m->dims[m->n_hidden + 1]);
        for (int l = 1; l <= m->n_hidden; l++)
            if (m->dims[l] < 1 || m->dims[l] > NET_MAX_WIDTH) return fail(nullptr, RANENV_E_INVALID, "hidden width %d (1..%d)", m->dims[l], NET_MAX_WIDTH);
        net[i].n_layers = m->n_hidden + 1;
        net_pack(m->dims, net[i].n_layers, RANENV_NET_F32, net[i], 0);
    }
    return RANENV_OK;
}

int ranenv_ppo_lds_bytes(const ranenv_mlp *actor, const ranenv_mlp *critic, int64_t *bytes)
{
    if (!actor || !bytes) return fail(nullptr, RANENV_E_INVALID, "null argument");
    PolicyNet net[2] = {};
    if (const int rc = ppo_shape_pair(actor, critic, net); rc != RANENV_OK) return rc;
    *bytes = (int64_t)ppo_lds_bytes(net[0], critic ? &net[1] : nullptr);
    return RANENV_OK;
}

int ranenv_ppo_wide_bytes(const ranenv_mlp *actor, const ranenv_mlp *critic, int64_t *lds_bytes, int64_t *scratch_floats)
{
    if (!actor || (!lds_bytes && !scratch_floats)) return fail(nullptr, RANENV_E_INVALID, "null argument");
    PolicyNet net[2] = {};
    if (const int rc = ppo_shape_pair(actor, critic, net); rc != RANENV_OK) return rc;
    if (lds_bytes) *lds_bytes = (int64_t)ppo_wide_lds_bytes(net[0], critic ? &net[1] : nullptr);
    if (scratch_floats) *scratch_floats = (int64_t)ppo_wide_scratch(net[0], critic ? &net[1] : nullptr);
    return RANENV_OK;
}

int ranenv_ppo_spread_bytes(const ranenv_mlp *actor, const ranenv_mlp *critic, int32_t slabs, int32_t wide, int64_t *bytes)
{
    if (!actor || !bytes) return fail(nullptr, RANENV_E_INVALID, "null argument");
    if (slabs < 1 || slabs > PPO_SPREAD_SLABS_MAX) return fail(nullptr, RANENV_E_INVALID, "slabs %d (1..256)", slabs);
    if (wide != 0 && wide != 1) return fail(nullptr, RANENV_E_INVALID, "wide %d (0 the LDS plan, 1 the wide plan)", wide);
    PolicyNet net[2] = {};
    if (const int rc = ppo_shape_pair(actor, critic, net); rc != RANENV_OK) return rc;
    const long long floats = net_floats(net[0]) + (critic ? net_floats(net[1]) : 0);
    *bytes = (int64_t)sizeof(float) * slabs * (floats + (wide ? ppo_wide_scratch(net[0], critic ? &net[1] : nullptr) : 0));
    return RANENV_OK;
}

int ranenv_ppo_slices_spread_bytes(const ranenv_mlp *inter_actor, const ranenv_mlp *inter_critic, const ranenv_mlp *intra_actor, const ranenv_mlp *intra_critic,
                                   int32_t n_slices, int32_t slabs, int32_t wide, int64_t *bytes)
{
    if (!inter_actor || !intra_actor || !bytes) return fail(nullptr, RANENV_E_INVALID, "null argument");
    if (n_slices < 1) return fail(nullptr, RANENV_E_INVALID, "n_slices %d (>= 1)", n_slices);
    int64_t inter = 0, intra = 0;
    if (const int rc = ranenv_ppo_spread_bytes(inter_actor, inter_critic, slabs, wide, &inter); rc != RANENV_OK) return rc;
    if (const int rc = ranenv_ppo_spread_bytes(intra_actor, intra_critic, slabs, wide, &intra); rc != RANENV_OK) return rc;
    *bytes = inter + (int64_t)n_slices * intra;
    return RANENV_OK;
}

int ranenv_ppo_spread_bfloat_bytes(const ranenv_mlp *actor, const ranenv_mlp *critic, int32_t slabs, int64_t *lds_bytes, int64_t *device_bytes)
{
    if (!actor || (!lds_bytes && !device_bytes)) return fail(nullptr, RANENV_E_INVALID, "null argument");
    if (slabs < 1 || slabs > PPO_SPREAD_SLABS_MAX) return fail(nullptr, RANENV_E_INVALID, "slabs %d (1..256)", slabs);
    PolicyNet net[2] = {};
    if (const int rc = ppo_shape_pair(actor, critic, net); rc != RANENV_OK) return rc;      // (kp, np: the same in either precision)
    if (lds_bytes) *lds_bytes = (int64_t)ppo_bf16_lds_bytes(net[0], critic ? &net[1] : nullptr);
    if (device_bytes) {      // slabs of the pair's f32 floats; per net master, m, v, g in f32 and the transposed bf16 weights beside its biases
        long long floats = 0, state = 0;
        for (int i = 0; i < (critic ? 2 : 1); i++) {
            const long long f32 = net_floats_f32(net[i]);
            long long w = 0;
            for (int l = 0; l < net[i].n_layers; l++) w += (long long)net[i].kp[l] * net[i].np[l];
            floats += f32; state += 4 * f32 + (f32 - w / 2);
        }
        *device_bytes = (int64_t)sizeof(float) * (slabs * floats + state);
    }
    return RANENV_OK;
}

int ranenv_ppo_spread_plan(int64_t n_rows, int32_t minibatch, int32_t epochs, int32_t slabs, int64_t *steps, int32_t *grid, int32_t *tiles_last)
{
    if (n_rows < 0 || n_rows > 0x7fffffffLL) return fail(nullptr, RANENV_E_INVALID, "n_rows %lld (0..2^31 - 1)", (long long)n_rows);
    if (minibatch < 1) return fail(nullptr, RANENV_E_INVALID, "minibatch %d (>= 1)", minibatch);
    if (epochs < 0) return fail(nullptr, RANENV_E_INVALID, "epochs %d (>= 0)", epochs);
    if (slabs < 1 || slabs > PPO_SPREAD_SLABS_MAX) return fail(nullptr, RANENV_E_INVALID, "slabs %d (1..256)", slabs);
    const int n = (int)n_rows, per_epoch = ppo_spread_per_epoch(n, minibatch);
    if (steps) *steps = (int64_t)epochs * per_epoch;
    if (grid) *grid = n > 0 ? ppo_spread_step(n, minibatch, slabs, 0).grid : 0;
    if (tiles_last) *tiles_last = n > 0 ? ppo_spread_step(n, minibatch, slabs, per_epoch - 1).tiles : 0;
    return RANENV_OK;
}

// The units' schedule of a per-slice spread call from its tables: ppo_slices_spread_unit and ppo_spread_step, the update's own functions
static void ppo_slices_spread_plan(const int (*first)[POP_MAX + 1], int n_units, int minibatch, int epochs, int slabs, int64_t *unit_steps, int32_t *unit_grid,
                                   int64_t *call_steps)
{
    int64_t most = 0;
    for (int u = 0; u < n_units; u++) {
        const PpoSliceUnit x = ppo_slices_spread_unit(first, u, 1, minibatch);      // (steps of ONE epoch: the product is taken in 64 bits here)
        const int64_t steps = (int64_t)epochs * x.steps;
        if (unit_steps) unit_steps[u] = steps;
        if (unit_grid) unit_grid[u] = x.n > 0 ? ppo_spread_step(x.n, minibatch, slabs, 0).grid : 0;
        most = std::max(most, steps);
    }
    if (call_steps) *call_steps = most;
}

int ranenv_ppo_slices_spread_plan(int32_t n_slices, int32_t n_inter, const int32_t *host_first_slice, int32_t minibatch, int32_t epochs, int32_t slabs,
                                  int64_t *unit_steps, int32_t *unit_grid, int64_t *call_steps)
{
    if (n_slices < 1 || n_slices > POP_MAX) return fail(nullptr, RANENV_E_INVALID, "n_slices %d (1..%d)", n_slices, (int)POP_MAX);
    if (n_inter < 0) return fail(nullptr, RANENV_E_INVALID, "n_inter %d (>= 0)", n_inter);
    if (!host_first_slice) return fail(nullptr, RANENV_E_INVALID, "null argument");
    if (minibatch < 1) return fail(nullptr, RANENV_E_INVALID, "minibatch %d (>= 1)", minibatch);
    if (epochs < 0) return fail(nullptr, RANENV_E_INVALID, "epochs %d (>= 0)", epochs);
    if (slabs < 1 || slabs > PPO_SPREAD_SLABS_MAX) return fail(nullptr, RANENV_E_INVALID, "slabs %d (1..256)", slabs);
    int first[2][POP_MAX + 1] = {};
    first[0][1] = n_inter;
    if (host_first_slice[0] != 0) return fail(nullptr, RANENV_E_INVALID, "host_first_slice[0] is %d, not 0", host_first_slice[0]);
    for (int s = 0; s < n_slices; s++) {
        if (host_first_slice[s + 1] < host_first_slice[s]) return fail(nullptr, RANENV_E_INVALID, "host_first_slice decreases at slice %d", s);
        first[1][s + 1] = host_first_slice[s + 1];
    }
    ppo_slices_spread_plan(first, 1 + n_slices, minibatch, epochs, slabs, unit_steps, unit_grid, call_steps);
    return RANENV_OK;
}

int ranenv_ppo_probe_logp(ranenv_handle h, float *dev_logp)
{
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    h->ppo_probe = dev_logp;
    return RANENV_OK;
}

// What an update needs of the record: the inter columns, the intra ones where the call trains `intra_actor`'s rows, rows an int32 numbers
static int ppo_record_check(ranenv_handle h, int32_t n_steps, const ranenv_trajectory *traj, const ranenv::NetSlot *intra_actor)
{
    if (!traj->obs_inter || !traj->mask_inter || !traj->action_inter || !traj->logp || !traj->adv || !traj->vtarg)
        return fail(h, RANENV_E_INVALID, "the record needs obs_inter, mask_inter, action_inter, logp, adv and vtarg");
    if (intra_actor && (!traj->obs_intra || !traj->action_intra || (intra_actor->net.layout == RANENV_NET_IN_MASK_OBS && !traj->mask_intra)))
        return fail(h, RANENV_E_INVALID, "the record needs obs_intra and action_intra (mask_intra for RANENV_NET_IN_MASK_OBS nets) for the intra rows");
    if ((long long)n_steps * h->cfg.batch * h->cfg.n_slices > 0x7fffffffLL) return fail(h, RANENV_E_INVALID, "the record has more than 2^31 - 1 intra rows");
    return RANENV_OK;
}

// ranenv_ppo_update under a spread binding: `a` as the update below filled it (nets, lists, record, counters, outputs).  Per kind the
// schedule's geometry and the kind's share of the binding's buffers, then three launches per optimiser step until the kind with more
// steps is through; a kind the call does not train, or whose list is empty, has no steps.
static int ppo_update_spread(ranenv_handle h, ranenv::NetSlot *const (&slot)[4], const PpoArgs &a, const ranenv_ppo_hparams &hp, bool intra, size_t lds, hipStream_t s)
{
    const ranenv::PpoBinding &b = h->ppo;
    PpoSpreadArgs p{};
    p.a = a; p.a.hp = nullptr; p.hp = hp; p.slabs = b.slabs;
    float *slab = h->d_ppo_slab, *park = h->d_ppo_park;
    long long steps = 0;
    for (int k = 0; k < 2; k++) {
        if (!slot[k]) continue;
        PpoSpreadKind &K = p.k[k];
        const PolicyNet *critic = slot[2 + k] ? &slot[2 + k]->net : nullptr;
        const long long floats = b.bf16 ? net_floats_f32(slot[k]->net) + (critic ? net_floats_f32(*critic) : 0)
                                        : net_floats(slot[k]->net) + (critic ? net_floats(*critic) : 0);
        K.slab = slab; K.slab_stride = floats; slab += floats * b.slabs;
        if (b.wide) { K.park = park; K.park_stride = ppo_wide_scratch(slot[k]->net, critic); park += K.park_stride * b.slabs; }
        K.bpart = h->d_ppo_spread + k * ppo_spread_doubles(h->ppo_spread_blocks);
        K.wstat = K.bpart + h->ppo_spread_blocks; K.run = K.wstat + PPO_SPREAD_SLABS_MAX * PPO_SPREAD_STATS;
        K.t0 = h->d_ppo_t + 2 + k;
        K.blocks = (int)((floats + PPO_SPREAD_BLOCK - 1) / PPO_SPREAD_BLOCK);
        if (k == 1 && !intra) continue;
        K.n = a.first[k][1];
        const long long k_steps = (long long)hp.epochs * ppo_spread_per_epoch(K.n, hp.minibatch);
        if (k_steps > 0x7fffffffLL) return fail(h, RANENV_E_INVALID, "%lld optimiser steps (epochs x minibatches of the %s kind): more than 2^31 - 1", k_steps, k ? "intra" : "inter");
        K.steps = (int)k_steps;
        steps = std::max(steps, k_steps);
    }
    if (b.bf16) {
        PpoSpreadBf16Args q{};
        q.p = p;
        for (int k = 0; k < 2; k++)
            for (int i = 0; i < 2; i++) q.bf[k][i] = ppo_bf16_net(h, slot[2 * i + k]);
        for (long long i = 0; i < steps; i++) {
            q.p.step = (int)i;
            HIP_TRY(h, launch_ppo_spread_step_bf16(s, lds, q));
        }
        return RANENV_OK;
    }
    for (long long i = 0; i < steps; i++) {
        p.step = (int)i;
        HIP_TRY(h, launch_ppo_spread_step(s, lds, p, b.wide));
    }
    return RANENV_OK;
}

// ranenv_ppo_update_slices under ranenv_ppo_bind_slices_spread: `a` as the update below filled it.  Per kind the buffers of its first
// unit and the strides between two slices', then three launches per optimiser step until the unit with most steps is through; the
// units' rows and steps follow from a.first and hp on the device as here (ppo_slices_spread_plan).
static int ppo_update_slices_spread(ranenv_handle h, ranenv::NetSlot *const (&slot)[4], const PpoArgs &a, const ranenv_ppo_hparams &hp, bool intra, size_t lds, hipStream_t s)
{
    const ranenv::PpoBinding &b = h->ppo;
    const int S = h->cfg.n_slices;
    PpoSpreadSlicesArgs q{};
    PpoSpreadArgs &p = q.p;
    p.a = a; p.a.hp = nullptr; p.hp = hp; p.slabs = b.slabs;
    q.x.n_units = intra ? 1 + S : 1;
    q.x.dbl_unit = ppo_spread_doubles(h->ppo_spread_blocks);
    float *slab = h->d_ppo_slab, *park = h->d_ppo_park;
    for (int k = 0; k < 2; k++) {
        PpoSpreadKind &K = p.k[k];
        const PolicyNet *critic = slot[2 + k] ? &slot[2 + k]->net : nullptr;
        const long long floats = net_floats(slot[k]->net) + (critic ? net_floats(*critic) : 0);
        const long long copies = (long long)b.slabs * (k ? S : 1);
        K.slab = slab; K.slab_stride = floats; slab += floats * copies;
        if (k) q.x.slab_unit = floats * b.slabs;
        if (b.wide) {
            K.park = park; K.park_stride = ppo_wide_scratch(slot[k]->net, critic); park += K.park_stride * copies;
            if (k) q.x.park_unit = K.park_stride * b.slabs;
        }
        K.bpart = h->d_ppo_spread + k * q.x.dbl_unit;      // (unit 0 and unit 1: slice s's lie s x dbl_unit behind the latter)
        K.wstat = K.bpart + h->ppo_spread_blocks; K.run = K.wstat + PPO_SPREAD_SLABS_MAX * PPO_SPREAD_STATS;
        K.t0 = h->d_ppo_t + POP_MAX + k;
        K.blocks = (int)((floats + PPO_SPREAD_BLOCK - 1) / PPO_SPREAD_BLOCK);
        K.steps = k == 0 || intra ? 1 : 0;
    }
    int64_t unit_steps[POP_MAX + 1], steps = 0;
    ppo_slices_spread_plan(p.a.first, q.x.n_units, hp.minibatch, hp.epochs, b.slabs, unit_steps, nullptr, &steps);
    for (int u = 0; u < q.x.n_units; u++)
        if (unit_steps[u] > 0x7fffffffLL) return fail(h, RANENV_E_INVALID, "%lld optimiser steps (epochs x minibatches of policy %d): more than 2^31 - 1", (long long)unit_steps[u], u);
    for (int64_t i = 0; i < steps; i++) {
        p.step = (int)i;
        HIP_TRY(h, launch_ppo_spread_slices_step(s, lds, q, b.wide));
    }
    return RANENV_OK;
}

// THE update behind ranenv_ppo_update and ranenv_ppo_update_slices, which bring their arguments into one form: per kind the row list
// `order[k]` (null: the kind is not trained) and `first[k]`, unit u's share [first[k][u], first[k][u + 1]) of every epoch's row of it
// -- the units of the binding's geometry -- and `n_hp` hyper-parameter sets, one per member (slices: one for all units).
static int ppo_update(ranenv_handle h, bool slices, int32_t n_steps, const ranenv_trajectory *traj, int32_t n_hp, const ranenv_ppo_hparams *hp,
                      const int32_t *const (&order)[2], const int32_t *const (&first)[2], double *stats, float *grad, void *stream)
{
    float *const probe_logp = h->ppo_probe;
    h->ppo_probe = nullptr;          // (armed for ONE update, served or refused: the handle keeps no caller's pointer beyond it)
    ranenv::NetSlot *slot[4];
    int members = 0;
    if (const int rc = ppo_bound(h, slices, slot, members); rc != RANENV_OK) return rc;
    const ranenv::PpoBinding &b = h->ppo;
    const int S = h->cfg.n_slices;
    if (n_steps < 1 || !traj || !hp || !order[0] || !first[0] || !stats)
        return fail(h, RANENV_E_INVALID, "n_steps >= 1, the record, the hyper-parameters, the inter row list%s and dev_stats are required", slices ? "" : "s");
    if (slices && first[0][1] < 0) return fail(h, RANENV_E_INVALID, "n_inter %d (>= 0)", first[0][1]);
    if (n_hp != members) return fail(h, RANENV_E_INVALID, "%d members given, the bound nets have %d", n_hp, members);
    const bool intra = order[1] != nullptr;
    if (intra && !first[1]) return fail(h, RANENV_E_INVALID, "intra row lists without host_first_%s", slices ? "slice" : "intra");
    if (intra && !slot[1]) return fail(h, RANENV_E_INVALID, "intra row lists but no intra actor is bound");
    int max_epochs = 0;
    for (int m = 0; m < n_hp; m++) {
        char whose[24] = "";
        if (!slices) snprintf(whose, sizeof(whose), "member %d: ", m);
        if (hp[m].minibatch < 1) return fail(h, RANENV_E_INVALID, "%sminibatch %d (>= 1)", whose, hp[m].minibatch);
        if (hp[m].epochs < 0) return fail(h, RANENV_E_INVALID, "%sepochs %d (>= 0)", whose, hp[m].epochs);
        max_epochs = hp[m].epochs > max_epochs ? hp[m].epochs : max_epochs;
    }
    if (const int rc = ppo_record_check(h, n_steps, traj, intra ? slot[1] : nullptr); rc != RANENV_OK) return rc;
    PpoArgs a{};
    for (int k = 0; k < (intra ? 2 : 1); k++) {
        const int units = b.units(k, members, S);
        const char *list = slices ? "slice" : (k ? "intra" : "inter");
        if (first[k][0] != 0) return fail(h, RANENV_E_INVALID, "host_first_%s[0] is %d, not 0", list, first[k][0]);
        for (int u = 0; u < units; u++)
            if (first[k][u + 1] < first[k][u]) return fail(h, RANENV_E_INVALID, "host_first_%s decreases at %s %d", list, slices ? "slice" : "member", u);
        for (int u = 0; u <= units; u++) a.first[k][u] = first[k][u];
        a.order[k] = order[k]; a.order_stride[k] = first[k][units];
        if (b.bf16) { a.net[k][0] = ppo_bf16_state(h, slot[k]); a.net[k][1] = ppo_bf16_state(h, slot[2 + k]); }
        else { a.net[k][0] = ppo_net(slot[k]); a.net[k][1] = ppo_net(slot[2 + k]); }
    }
    if (max_epochs == 0) return RANENV_OK;
    a.T = n_steps; a.B = h->cfg.batch; a.S = S; a.Us = h->cfg.max_ues_slice; a.W = 2 * a.Us + 9;
    a.hp = h->d_ppo_hp; a.traj = *traj; a.t = h->d_ppo_t; a.max_epochs = max_epochs; a.stats = stats; a.grad = grad; a.probe_logp = probe_logp;
    // The launch's LDS: the largest need over the kinds this call updates (a mixed binding: and over the members).  dev_grad's stride
    // is ranenv_ppo_layout's: the largest of the BOUND nets, whether or not this call updates the intra kind
    const PpoPlan plan = ppo_plan(slot, b.mixed, b.wide, members, intra ? 2 : 1, b.bf16);
    a.grad_stride = plan.grad_floats;
    PpoMixed x{};
    if (b.mixed) {      // (every bound role is the population's: its table; the others the table of zeros)
        for (int k = 0; k < 2; k++)
            for (int i = 0; i < 2; i++) x.tab[k][i] = h->d_pop_tab + (slot[2 * i + k] ? 2 * i + k : 4) * POP_MAX;
        x.floats = h->d_ppo_floats;
    }
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    if (b.slabs && slices) return ppo_update_slices_spread(h, slot, a, hp[0], intra, plan.lds, s);
    if (b.slabs) return ppo_update_spread(h, slot, a, hp[0], intra, plan.lds, s);
    HIP_TRY(h, hipMemcpyAsync(h->d_ppo_hp, hp, sizeof(ranenv_ppo_hparams) * (size_t)n_hp, hipMemcpyHostToDevice, s));
    const PpoWide y{h->d_ppo_park, h->ppo_park_stride};      // (ppo_bound: every workgroup's rows fit its share)
    if (slices) HIP_TRY(h, launch_ppo_update_slices(s, intra ? S : 0, plan.lds, a, b.wide ? &y : nullptr));
    else HIP_TRY(h, launch_ppo_update(s, members, plan.lds, a, b.mixed ? &x : nullptr, b.wide ? &y : nullptr));
    return RANENV_OK;
}

int ranenv_ppo_update(ranenv_handle h, int32_t n_steps, const ranenv_trajectory *traj, int32_t n_members, const ranenv_ppo_hparams *hp,
                      const int32_t *order_inter, const int32_t *first_inter, const int32_t *order_intra, const int32_t *first_intra, double *stats,
                      float *grad, void *stream)
{
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    const int32_t *const order[2] = {order_inter, order_intra}, *const first[2] = {first_inter, first_intra};
    return ppo_update(h, false, n_steps, traj, n_members, hp, order, first, stats, grad, stream);
}

// ranenv_ppo_update_slices: the per-slice geometry -- unit s of kind 1 is slice s, and the one inter unit's share is all n_inter rows
int ranenv_ppo_update_slices(ranenv_handle h, int32_t n_steps, const ranenv_trajectory *traj, const ranenv_ppo_hparams *hp, const int32_t *order_inter,
                             int32_t n_inter, const int32_t *order_intra, const int32_t *first_slice, double *stats, float *grad, void *stream)
{
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    const int32_t first_inter[2] = {0, n_inter};
    const int32_t *const order[2] = {order_inter, order_intra}, *const first[2] = {first_inter, first_slice};
    return ppo_update(h, true, n_steps, traj, 1, hp, order, first, stats, grad, stream);
}

// A role's slot and the float offset of slice `slice`'s copy in it, for ranenv_get_slice_net_weights (roles 1 and 3 alone) and
// ranenv_ppo_slice_state (roles 0 and 2: offset 0, `slice` ignored)
static int slice_copy(ranenv_handle h, int32_t role, int32_t slice, bool intra_only, ranenv::NetSlot *&slot, size_t &at)
{
    if (const int rc = role_check(h, role); rc != RANENV_OK) return rc;
    slot = h->serving(role); at = 0;
    if (!slot) return fail(h, RANENV_E_STATE, "no %s net bound", NET_ROLES[role].who);
    if (!(role & 1)) return intra_only ? fail(h, RANENV_E_INVALID, "role %d: the nets per slice are roles 1 (intra actors) and 3 (intra critics)", role) : (int)RANENV_OK;
    if (slot->form != FORM_SLICE) return fail(h, RANENV_E_STATE, "the %s nets are not bound per slice", NET_ROLES[role].who);
    if (slice < 0 || slice >= h->cfg.n_slices) return fail(h, RANENV_E_INVALID, "slice %d outside the %d", slice, h->cfg.n_slices);
    at = (size_t)slice * (size_t)slot->net.slice_stride;
    return RANENV_OK;
}

// ranenv_ppo_state / ranenv_ppo_slice_state: unit `u`'s copy of `role`'s net in the bound state of that geometry -- the slot, the
// float offset of the copy in it and the unit's step counter
static int ppo_state_at(ranenv_handle h, bool slices, int32_t role, int32_t u, ranenv::NetSlot *&x, size_t &at, int32_t *&t)
{
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    if (const int rc = role_check(h, role); rc != RANENV_OK) return rc;
    ranenv::NetSlot *slot[4];
    int members = 0;
    if (const int rc = ppo_bound(h, slices, slot, members); rc != RANENV_OK) return rc;
    if (slices) {
        if (const int rc = slice_copy(h, role, u, false, x, at); rc != RANENV_OK) return rc;
    } else {
        if (u < 0 || u >= members) return fail(h, RANENV_E_INVALID, "member %d outside the %d", u, members);
        if (!slot[role]) return fail(h, RANENV_E_STATE, "no %s net bound", NET_ROLES[role].who);
        x = slot[role]; at = (size_t)u * (size_t)x->member_stride;
    }
    t = h->d_ppo_t + h->ppo.wg(role & 1, u);
    return RANENV_OK;
}

int ranenv_ppo_state(ranenv_handle h, int32_t role, int32_t member, float **dev_m, float **dev_v, int32_t **dev_t, int64_t *floats)
{
    ranenv::NetSlot *x = nullptr; size_t at = 0; int32_t *t = nullptr;
    if (const int rc = ppo_state_at(h, false, role, member, x, at, t); rc != RANENV_OK) return rc;
    if (h->ppo.bf16) {      // (the moments of a bf16 net lie beside its f32 master, in the F32 packed layout)
        const PpoNet n = ppo_bf16_state(h, x);
        if (dev_m) *dev_m = n.m;
        if (dev_v) *dev_v = n.v;
        if (dev_t) *dev_t = t;
        if (floats) *floats = n.floats;
        return RANENV_OK;
    }
    if (dev_m) *dev_m = x->opt + at;
    if (dev_v) *dev_v = x->opt + x->opt_cap + at;
    if (dev_t) *dev_t = t;
    if (floats) *floats = net_floats(x->member[h->ppo.mixed ? (size_t)member : 0]);
    return RANENV_OK;
}

int ranenv_ppo_slice_state(ranenv_handle h, int32_t role, int32_t slice, float **dev_m, float **dev_v, int32_t **dev_t, int64_t *floats)
{
    ranenv::NetSlot *x = nullptr; size_t at = 0; int32_t *t = nullptr;
    if (const int rc = ppo_state_at(h, true, role, slice, x, at, t); rc != RANENV_OK) return rc;
    if (dev_m) *dev_m = x->opt + at;
    if (dev_v) *dev_v = x->opt + x->opt_cap + at;
    if (dev_t) *dev_t = t;
    if (floats) *floats = net_floats(x->net);
    return RANENV_OK;
}

// Copy `member` of `slot` (`who` for the messages) unpacked to torch Linear layout: ranenv_get_net_weights / ranenv_get_head_net_weights
// master: a bf16 net's f32 master copy under ranenv_ppo_bind_spread_bfloat, in the F32 packed layout -- the one form of a bf16 net that exports
static int net_export(ranenv_handle h, const ranenv::NetSlot *slot, int member, const char *who, ranenv_mlp *out, void *stream, const float *packed = nullptr,
                      const float *master = nullptr)
{
    PolicyNet net = slot->member[(size_t)member];
    if (master) {
        PpoBf16Net f32{};
        net_floats_f32(net, &f32);
        for (int l = 0; l < net.n_layers; l++) { net.w_off[l] = f32.w_off[l]; net.b_off[l] = f32.b_off[l]; }
        net.prec = RANENV_NET_F32; packed = master;
    }
    if (net.prec != RANENV_NET_F32) return fail(h, RANENV_E_STATE, "the %s net is bf16: its float32 weights were rounded at bind", who);
    const int32_t *dims = slot->member_dims[(size_t)member].data();
    const int L = net.n_layers;
    for (int l = 0; l < L; l++)
        if ((out->weight[l] == nullptr) != (out->weight[0] == nullptr) || (out->bias[l] == nullptr) != (out->weight[0] == nullptr))
            return fail(h, RANENV_E_INVALID, "give every layer's weight and bias buffer, or none");
    const bool copy = out->weight[0] != nullptr;
    out->n_hidden = L - 1; out->activation = net.act; out->input_layout = net.layout; out->precision = slot->member[(size_t)member].prec;
    for (int l = 0; l < 6; l++) out->dims[l] = l <= L ? dims[l] : 0;
    if (!copy) return RANENV_OK;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    const float *src = packed ? packed : net.w;      // (packed: another copy in the slot's layout -- the SAC binding's live critics)
    for (int l = 0; l < L; l++) {
        const int K = dims[l], N = dims[l + 1];
        HIP_TRY(h, hipMemcpy2DAsync((void *)out->weight[l], sizeof(float) * K, src + net.w_off[l], sizeof(float) * net.kp[l], sizeof(float) * K, N, hipMemcpyDeviceToDevice, s));
        HIP_TRY(h, hipMemcpyAsync((void *)out->bias[l], src + net.b_off[l], sizeof(float) * N, hipMemcpyDeviceToDevice, s));
    }
    return RANENV_OK;
}

int ranenv_get_net_weights(ranenv_handle h, int32_t role, int32_t member, ranenv_mlp *out, void *stream)
{
    if (!h || !out) return fail(h, RANENV_E_INVALID, "null argument");
    if (const int rc = role_check(h, role); rc != RANENV_OK) return rc;
    const ranenv::NetSlot *slot = h->serving(role);
    if (!slot) return fail(h, RANENV_E_STATE, "no %s net bound", NET_ROLES[role].who);
    if (slot->form == FORM_SLICE) return fail(h, RANENV_E_STATE, "the %s nets are bound per slice", NET_ROLES[role].who);
    const int members = (int)slot->member.size();
    if (member < 0 || member >= members) return fail(h, RANENV_E_INVALID, "member %d outside the %d", member, members);
    const bool master = h->ppo.on && h->ppo.bf16 && slot->form == FORM_ONE && ppo_bf16_fits(h, slot);
    return net_export(h, slot, member, NET_ROLES[role].who, out, stream, nullptr, master ? h->d_ppo_bf[role] : nullptr);
}

int ranenv_get_slice_net_weights(ranenv_handle h, int32_t role, int32_t slice, ranenv_mlp *out, void *stream)
{
    if (!h || !out) return fail(h, RANENV_E_INVALID, "null argument");
    ranenv::NetSlot *slot = nullptr;
    size_t at = 0;
    if (const int rc = slice_copy(h, role, slice, true, slot, at); rc != RANENV_OK) return rc;
    return net_export(h, slot, 0, NET_ROLES[role].who, out, stream, slot->w + at);      // (slice 0's entry is every slice's layout)
}

// ---- PPO update of the head policies (include/ranenv.h "PPO update of the head policies"; ranenv_ppo_update_kernel_head) -----------
// What ranenv_ppo_bind_head refuses.  No device call.
static int ppo_head_roles(ranenv_handle h, size_t &lds)
{
    if (!h->head.on || !h->head_value.on)
        return fail(h, RANENV_E_STATE, "the head PPO update needs a bound head actor and head critic (ranenv_set_head_policy_network, ranenv_set_head_value_network)");
    if (h->head_dist != RANENV_HEAD_DIST_GAUSS_CLIP) return fail(h, RANENV_E_STATE, "the head PPO update trains GAUSS_CLIP (PPO) policies: the head actor is GAUSS_TANH");
    if (h->head.net.prec != RANENV_NET_F32) return fail(h, RANENV_E_STATE, "the PPO update trains float32 nets: the head net is bf16");
    if (h->head_value.net.prec != RANENV_NET_F32) return fail(h, RANENV_E_STATE, "the PPO update trains float32 nets: the head value net is bf16");
    lds = ppo_lds_bytes(h->head.net, &h->head_value.net);
    if (lds > (size_t)PPO_LDS_MAX)
        return fail(h, RANENV_E_STATE, "the head nets need %zu bytes of LDS for their 32-row activations of all layers, the update has %d", lds, (int)PPO_LDS_MAX);
    return RANENV_OK;
}

// What the spread head binding holds beside the moments, for the head nets as they stand: floats of gradient slabs and reduce / apply blocks
struct PpoHeadSpreadNeed { long long floats, slab, blocks; };
static PpoHeadSpreadNeed ppo_head_spread_need(ranenv_handle h, int slabs)
{
    PpoHeadSpreadNeed n{};
    n.floats = net_floats(h->head.net) + net_floats(h->head_value.net);
    n.slab = n.floats * slabs;
    n.blocks = (n.floats + PPO_SPREAD_BLOCK - 1) / PPO_SPREAD_BLOCK;
    return n;
}
static long long ppo_head_spread_doubles(long long blocks, int slabs, int S) { return (long long)slabs * S + blocks + PPO_SPREAD_SLABS_MAX * PPO_SPREAD_STATS + RANENV_PPO_STATS; }

// ... and the bound state behind it, or RANENV_E_STATE
static int ppo_head_bound(ranenv_handle h, size_t &lds)
{
    if (!h->ppo_head_on) return fail(h, RANENV_E_STATE, "no head PPO state bound, or a binding call has outgrown it (ranenv_ppo_bind_head)");
    if (const int rc = ppo_head_roles(h, lds); rc != RANENV_OK) return rc;
    for (const ranenv::NetSlot *x : {&h->head, &h->head_value})
        if (!x->opt || x->opt_cap < x->cap) return fail(h, RANENV_E_STATE, "a head net was bound after ranenv_ppo_bind_head: bind again");
    if (h->ppo_head_slabs) {      // the spread form: the slabs and block partials of the nets as they stand fit what the bind allocated
        const PpoHeadSpreadNeed need = ppo_head_spread_need(h, h->ppo_head_slabs);
        if (need.slab > h->ppo_head_slab_cap || need.blocks > h->ppo_head_blocks || h->ppo_head_slabs > h->ppo_head_gls_slabs)
            return fail(h, RANENV_E_STATE, "the head nets need more slab floats than ranenv_ppo_bind_head_spread allocated: bind again");
    }
    return RANENV_OK;
}

// A binding call has replaced the head actor or the head critic: the moments of both nets and of log_std and the one counter start
// again, on the caller's stream -- or, where the slot has no moments of its size, the head binding ends.
static int ppo_head_rebound(ranenv_handle h, ranenv::NetSlot *slot, hipStream_t s)
{
    if (!h->ppo_head_on) return RANENV_OK;
    if (!slot->opt || slot->cap > slot->opt_cap) { h->ppo_head_on = false; return RANENV_OK; }
    for (ranenv::NetSlot *x : {&h->head, &h->head_value})
        if (x->on && x->opt && x->cap <= x->opt_cap) HIP_TRY(h, hipMemsetAsync(x->opt, 0, sizeof(float) * 2 * (size_t)x->opt_cap, s));
    HIP_TRY(h, hipMemsetAsync(h->d_head_ls_opt, 0, sizeof(float) * 2 * (size_t)h->cfg.n_slices, s));
    HIP_TRY(h, hipMemsetAsync(h->d_ppo_head_t, 0, sizeof(int32_t), s));
    return RANENV_OK;
}

// ranenv_ppo_bind_head (slabs 0) / ranenv_ppo_bind_head_spread (slabs 1..256): the later one replaces the earlier and restarts the optimiser
static int ppo_bind_head(ranenv_handle h, int slabs, void *stream)
{
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    size_t lds = 0;
    if (const int rc = ppo_head_roles(h, lds); rc != RANENV_OK) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    const size_t S = (size_t)h->cfg.n_slices;
    if (slabs) {      // the spread form's own: slabs (zeroed), gls, block partials, slab statistics and running sums
        const PpoHeadSpreadNeed need = ppo_head_spread_need(h, slabs);
        if (h->ppo_head_slab_cap < need.slab) {
            if (const int rc = dev_alloc(h, &h->d_ppo_head_slab, (size_t)need.slab); rc != RANENV_OK) return rc;
            h->ppo_head_slab_cap = need.slab;
        }
        if (!h->d_ppo_head_spread || h->ppo_head_blocks < need.blocks || h->ppo_head_gls_slabs < slabs) {
            const long long blocks = std::max(need.blocks, h->ppo_head_blocks);
            const int gls = std::max(slabs, h->ppo_head_gls_slabs);
            if (const int rc = dev_alloc(h, &h->d_ppo_head_spread, (size_t)ppo_head_spread_doubles(blocks, gls, (int)S)); rc != RANENV_OK) return rc;
            h->ppo_head_blocks = blocks; h->ppo_head_gls_slabs = gls;
        }
        HIP_TRY(h, hipMemsetAsync(h->d_ppo_head_slab, 0, sizeof(float) * (size_t)h->ppo_head_slab_cap, s));
    }
    if (!h->d_ppo_head_t) {
        if (const int rc = dev_alloc(h, &h->d_ppo_head_t, (size_t)2); rc != RANENV_OK) return rc;
        if (const int rc = dev_alloc(h, &h->d_head_ls_opt, 3 * S); rc != RANENV_OK) return rc;
    }
    HIP_TRY(h, hipMemsetAsync(h->d_ppo_head_t, 0, sizeof(int32_t), s));
    HIP_TRY(h, hipMemsetAsync(h->d_head_ls_opt, 0, sizeof(float) * 3 * S, s));
    for (ranenv::NetSlot *x : {&h->head, &h->head_value})
        if (const int rc = opt_ensure(h, x, s); rc != RANENV_OK) return rc;
    h->ppo_head_on = true;
    h->ppo_head_slabs = slabs;
    return RANENV_OK;
}

int ranenv_ppo_bind_head(ranenv_handle h, void *stream) { return ppo_bind_head(h, 0, stream); }
// (the head policies over the chip, include/ranenv.h "Head policies over the chip")
int ranenv_ppo_bind_head_spread(ranenv_handle h, int32_t slabs, void *stream)
{
    if (slabs < 1 || slabs > PPO_SPREAD_SLABS_MAX) return fail(h, RANENV_E_INVALID, "slabs %d (1..256)", slabs);
    return ppo_bind_head(h, slabs, stream);
}

int ranenv_ppo_head_spread_bytes(const ranenv_mlp *actor, const ranenv_mlp *critic, int32_t n_slices, int32_t slabs, int64_t *bytes)
{
    if (!actor || !critic || !bytes) return fail(nullptr, RANENV_E_INVALID, "null argument");
    if (n_slices < 1 || n_slices > 16) return fail(nullptr, RANENV_E_INVALID, "n_slices %d (1..16)", n_slices);
    if (slabs < 1 || slabs > PPO_SPREAD_SLABS_MAX) return fail(nullptr, RANENV_E_INVALID, "slabs %d (1..256)", slabs);
    PolicyNet net[2] = {};
    if (const int rc = ppo_shape_pair(actor, critic, net); rc != RANENV_OK) return rc;
    *bytes = (int64_t)slabs * ((int64_t)sizeof(float) * (net_floats(net[0]) + net_floats(net[1])) + (int64_t)sizeof(double) * n_slices);
    return RANENV_OK;
}

int ranenv_ppo_head_layout(ranenv_handle h, int64_t *actor_floats, int64_t *critic_floats, int64_t *lds_bytes)
{
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    size_t lds = 0;
    if (const int rc = ppo_head_roles(h, lds); rc != RANENV_OK) return rc;
    if (actor_floats) *actor_floats = net_floats(h->head.net);
    if (critic_floats) *critic_floats = net_floats(h->head_value.net);
    if (lds_bytes) *lds_bytes = (int64_t)lds;
    return RANENV_OK;
}

int ranenv_ppo_head_state(ranenv_handle h, int32_t which, float **dev_m, float **dev_v, int32_t **dev_t, int64_t *floats)
{
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    if (which < 0 || which > 2) return fail(h, RANENV_E_INVALID, "which %d (0 actor, 1 critic, 2 log_std)", which);
    size_t lds = 0;
    if (const int rc = ppo_head_bound(h, lds); rc != RANENV_OK) return rc;
    const ranenv::NetSlot *x = which == 0 ? &h->head : &h->head_value;
    const long long S = h->cfg.n_slices;
    if (dev_m) *dev_m = which == 2 ? h->d_head_ls_opt : x->opt;
    if (dev_v) *dev_v = which == 2 ? h->d_head_ls_opt + S : x->opt + x->opt_cap;
    if (dev_t) *dev_t = h->d_ppo_head_t;
    if (floats) *floats = which == 2 ? S : net_floats(x->net);
    return RANENV_OK;
}

int ranenv_ppo_update_head(ranenv_handle h, int32_t n_steps, const ranenv_head_trajectory *traj, const ranenv_ppo_hparams *hp, const int32_t *order,
                           int32_t n_rows, int32_t max_epochs, double *stats, float *grad, void *stream)
{
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    size_t lds = 0;
    if (const int rc = ppo_head_bound(h, lds); rc != RANENV_OK) return rc;
    if (n_steps < 1 || !traj || !hp || !order || !stats || n_rows < 0 || max_epochs < 0)
        return fail(h, RANENV_E_INVALID, "n_steps >= 1, the record, the hyper-parameters, the row lists (n_rows >= 0, max_epochs >= 0) and dev_stats are required");
    if (hp->minibatch < 1) return fail(h, RANENV_E_INVALID, "minibatch %d (>= 1)", hp->minibatch);
    if (hp->epochs < 0) return fail(h, RANENV_E_INVALID, "epochs %d (>= 0)", hp->epochs);
    if (hp->epochs > max_epochs) return fail(h, RANENV_E_INVALID, "epochs %d, the row lists and dev_stats have %d", hp->epochs, max_epochs);
    if (!traj->obs_head || !traj->action || !traj->logp || !traj->adv || !traj->vtarg)
        return fail(h, RANENV_E_INVALID, "the record needs obs_head, action, logp, adv and vtarg");
    if ((long long)n_steps * h->cfg.batch > 0x7fffffffLL) return fail(h, RANENV_E_INVALID, "the record has more than 2^31 - 1 rows");
    if (hp->epochs == 0 || n_rows == 0) return RANENV_OK;
    PpoHeadArgs a{};
    a.net[0] = ppo_net(&h->head); a.net[1] = ppo_net(&h->head_value);
    const int S = h->cfg.n_slices;
    a.log_std = h->d_head_log_std; a.ls_m = h->d_head_ls_opt; a.ls_v = a.ls_m + S; a.ls_g = a.ls_v + S;
    a.order = order; a.n_rows = n_rows; a.T = n_steps; a.B = h->cfg.batch; a.S = S;
    a.hp = *hp; a.traj = *traj; a.t = h->d_ppo_head_t; a.stats = stats; a.grad = grad;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    if (!h->ppo_head_slabs) {
        HIP_TRY(h, launch_ppo_update_head((hipStream_t)stream, lds, a));
        return RANENV_OK;
    }
    // the spread form: three launches per optimiser step on the head binding's own buffers
    const long long steps = (long long)hp->epochs * ppo_spread_per_epoch(n_rows, hp->minibatch);
    if (steps > 0x7fffffffLL) return fail(h, RANENV_E_INVALID, "%lld optimiser steps (epochs x minibatches): more than 2^31 - 1", steps);
    PpoHeadSpreadArgs p{};
    p.a = a;
    PpoHeadSpread &K = p.k;
    K.slabs = h->ppo_head_slabs; K.steps = (int)steps;
    K.slab = h->d_ppo_head_slab; K.slab_stride = a.net[0].floats + a.net[1].floats;
    K.blocks = (int)((K.slab_stride + PPO_SPREAD_BLOCK - 1) / PPO_SPREAD_BLOCK);
    K.gls = h->d_ppo_head_spread; K.bpart = K.gls + (size_t)h->ppo_head_gls_slabs * S;
    K.wstat = K.bpart + h->ppo_head_blocks; K.run = K.wstat + PPO_SPREAD_SLABS_MAX * PPO_SPREAD_STATS;
    K.t0 = h->d_ppo_head_t + 1;
    for (long long i = 0; i < steps; i++) {
        K.step = (int)i;
        HIP_TRY(h, launch_ppo_spread_head_step((hipStream_t)stream, lds, p));
    }
    return RANENV_OK;
}

int ranenv_get_head_net_weights(ranenv_handle h, int32_t which, ranenv_mlp *out, void *stream)
{
    if (!h || !out) return fail(h, RANENV_E_INVALID, "null argument");
    if (which != 0 && which != 1) return fail(h, RANENV_E_INVALID, "which %d (0 actor, 1 critic)", which);
    const ranenv::NetSlot *slot = which == 0 ? &h->head : &h->head_value;
    const char *who = which == 0 ? "head" : "head value";
    if (!slot->on) return fail(h, RANENV_E_STATE, "no %s net bound", who);
    return net_export(h, slot, 0, who, out, stream);
}

int ranenv_get_head_log_std(ranenv_handle h, float *dev_out, void *stream)
{
    if (!h || !dev_out) return fail(h, RANENV_E_INVALID, "null argument");
    if (!h->head.on || h->head_dist != RANENV_HEAD_DIST_GAUSS_CLIP) return fail(h, RANENV_E_STATE, "no GAUSS_CLIP head actor bound: the handle holds no log_std");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipMemcpyAsync(dev_out, h->d_head_log_std, sizeof(float) * (size_t)h->cfg.n_slices, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return RANENV_OK;
}

int ranenv_set_head_policy_network(ranenv_handle h, const ranenv_mlp *actor, int32_t dist, const float *dev_log_std, int32_t stochastic,
                                   uint64_t seed, void *stream_)
{
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    if (!actor) return fail(h, RANENV_E_INVALID, "the head actor is required");
    if (dist != RANENV_HEAD_DIST_GAUSS_CLIP && dist != RANENV_HEAD_DIST_GAUSS_TANH) return fail(h, RANENV_E_INVALID, "unknown head distribution %d", dist);
    if (dist == RANENV_HEAD_DIST_GAUSS_CLIP && !dev_log_std) return fail(h, RANENV_E_INVALID, "GAUSS_CLIP needs dev_log_std [S]");
    if (dist == RANENV_HEAD_DIST_GAUSS_TANH && dev_log_std) return fail(h, RANENV_E_INVALID, "GAUSS_TANH takes log_std from the net: dev_log_std must be NULL");
    const size_t S = (size_t)h->cfg.n_slices;
    hipStream_t s = (hipStream_t)stream_;
    NetBind b{&h->head, &actor, 1, dist == RANENV_HEAD_DIST_GAUSS_TANH ? NET_HEAD_TANH : NET_HEAD_CLIP};
    int rc = net_plan(h, &b, 1);
    if (rc != RANENV_OK) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    if ((rc = net_action_buffers(h)) != RANENV_OK) return rc;
    if (!h->d_head_log_std && (rc = dev_alloc(h, &h->d_head_log_std, S)) != RANENV_OK) return rc;
    if (dev_log_std) HIP_TRY(h, hipMemcpyAsync(h->d_head_log_std, dev_log_std, sizeof(float) * S, hipMemcpyDeviceToDevice, s));
    if ((rc = net_commit(h, &b, 1, s)) != RANENV_OK) return rc;
    h->head_dist = dist; h->head_stochastic = stochastic != 0; h->head_seed = seed;
    return RANENV_OK;
}

int ranenv_set_head_value_network(ranenv_handle h, const ranenv_mlp *critic, void *stream)
{
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    if (!critic) return fail(h, RANENV_E_INVALID, "the head critic is required");
    NetBind b{&h->head_value, &critic, 1, NET_HEAD_VALUE};
    if (const int rc = net_plan(h, &b, 1); rc != RANENV_OK) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    return net_commit(h, &b, 1, (hipStream_t)stream);
}

int ranenv_set_head_policy_source(ranenv_handle h, int32_t source)
{
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    if (source != RANENV_HEAD_SRC_HEAD && source != RANENV_HEAD_SRC_INTER) return fail(h, RANENV_E_INVALID, "unknown head policy source %d", source);
    if (source == h->head_src) return RANENV_OK;
    h->head_src = source;
    h->ring = ranenv_replay{}; h->ring_on = false; h->ring_written = 0;      // (its reward rows change width)
    return RANENV_OK;
}

static int check_ready(ranenv_handle h, const float *se_tiles, const double *traffic_bits, bool need_traffic)
{
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    if (!h->have_scenarios) return fail(h, RANENV_E_STATE, "no scenarios loaded (ranenv_load_scenarios)");
    if (!h->have_episodes) return fail(h, RANENV_E_STATE, "no episode descriptors (ranenv_set_episodes)");
    // (a handle whose sidecars came straight from power -- ranenv_bind_se_gather_from_power -- replays tiles without an RB-major pool)
    if (!se_tiles && !h->kp.se_pool && !(h->se_mode == RANENV_SE_GATHER && h->d_se_mean))
        return fail(h, RANENV_E_STATE, "no SE tiles given and no SE pool bound");
    if (need_traffic && !traffic_bits && !h->kp.trf_pool && !h->kp.trf_gen)
        return fail(h, RANENV_E_STATE, "no traffic given, no traffic pool bound and no traffic generator set");
    return RANENV_OK;
}

static int check_part(ranenv_handle h, int32_t part)
{
    if (part < 0 || part >= h->n_parts || h->part_lo.empty()) return fail(h, RANENV_E_INVALID, "partition %d outside [0,%d) (ranenv_set_partitions)", part, h->n_parts);
    return RANENV_OK;
}

// The partition's stream picks up behind what the caller's stream holds now (the producer of the scores) -- unless the
// caller works on the partition's stream itself (ranenv_get_part_stream): then stream order is all that is needed, and
// no signal crosses between hardware queues (a cross-queue dependency costs ~15 us each way on this GPU)
static int part_handoff(ranenv_handle h, int32_t part, hipStream_t stream)
{
    hipStream_t ps = h->part_stream[(size_t)part];
    if (stream != ps) {
        HIP_TRY(h, hipEventRecord(h->part_in[(size_t)part], stream));
        HIP_TRY(h, hipStreamWaitEvent(ps, h->part_in[(size_t)part], 0));
    }
    return RANENV_OK;
}

// What ranenv_step and ranenv_step_range open with, for envs [env_first, env_first + env_count): the checks, the call's KP with
// compact steps decided, and under RANENV_POLICY_NETWORK the nets' launch, whose status lands in *net_err (the callers word its
// failure differently).
static int step_begin(ranenv_handle h, int32_t env_first, int32_t env_count, const double *scores, const uint8_t *intra,
                      const double *traffic_bits, const float *se_tiles, float *obs_inter, float *obs_intra, double *reward,
                      uint8_t *done, hipStream_t stream, KP *kp, hipError_t *net_err)
{
    int rc = check_ready(h, se_tiles, traffic_bits, true);
    if (rc != RANENV_OK) return rc;
    if (env_first < 0 || env_count < 1 || (long long)env_first + env_count > h->cfg.batch)
        return fail(h, RANENV_E_INVALID, "envs [%d,%d) outside the batch of %d", env_first, env_first + env_count, h->cfg.batch);
    if (!scores && h->kp.policy == RANENV_POLICY_EXTERNAL) return fail(h, RANENV_E_STATE, "policy is EXTERNAL but no inter-slice scores were given");
    rc = slice_metrics_outputs(h, obs_intra, reward);
    if (rc != RANENV_OK) return rc;
    rc = trace_outputs(h, se_tiles, obs_inter, obs_intra, reward, done);
    if (rc != RANENV_OK) return rc;
    *kp = call_kp(h, obs_inter, obs_intra, reward, done);
    kp->se_tiles = se_tiles; kp->scores = scores; kp->intra = intra; kp->traffic_bits = traffic_bits;
    const int net = net_use(h, *kp);
    if (net < 0) return net;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    rc = compact_for(h, *kp, stream, &kp->compact);
    if (rc != RANENV_OK) return rc;
    *net_err = net ? net_launch(h, *kp, env_first, env_count, stream) : hipSuccess;
    return RANENV_OK;
}

int ranenv_reset(ranenv_handle h, const uint8_t *env_mask, const float *se_tiles, float *obs_inter, float *obs_intra,
                 double *reward, void *stream)
{
    int rc = check_ready(h, se_tiles, nullptr, false);
    if (rc != RANENV_OK) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    KP kp = call_kp(h, obs_inter, obs_intra, reward, nullptr);
    kp.env_mask = env_mask; kp.se_tiles = se_tiles;
    hipError_t e = launch<MODE_RESET>(h, kp, (hipStream_t)stream);
    if (e != hipSuccess) return fail(h, RANENV_E_HIP, "reset launch: %s", hipGetErrorString(e));
    if (env_mask == nullptr) h->idle_state_clean = true;        // every queue of the batch is empty again
    if (env_mask == nullptr) { h->sh_steps.assign((size_t)h->cfg.batch, 0); h->sh_valid = true; }
    else h->sh_valid = false;                                   // (which envs restart is on the device)
    return RANENV_OK;
}

int ranenv_step(ranenv_handle h, const double *scores, const uint8_t *intra, const double *traffic_bits,
                const float *se_tiles, float *obs_inter, float *obs_intra, double *reward, uint8_t *done, void *stream)
{
    KP kp;
    hipError_t e;
    const int rc = step_begin(h, 0, h ? h->cfg.batch : 0, scores, intra, traffic_bits, se_tiles, obs_inter, obs_intra, reward, done,
                              (hipStream_t)stream, &kp, &e);
    if (rc != RANENV_OK) return rc;
    if (e != hipSuccess) return fail(h, RANENV_E_HIP, "policy network launch: %s", hipGetErrorString(e));
    e = launch<MODE_STEP>(h, kp, (hipStream_t)stream);
    if (e != hipSuccess) return fail(h, RANENV_E_HIP, "step launch: %s", hipGetErrorString(e));
    shadow_steps_add(h, 0, h->cfg.batch, 1, done, (hipStream_t)stream);
    return RANENV_OK;
}

int ranenv_step_dense(ranenv_handle h, const uint8_t *dense, const double *traffic_bits, const float *se_tiles,
                      float *obs_inter, float *obs_intra, double *reward, uint8_t *done, void *stream)
{
    int rc = check_ready(h, se_tiles, traffic_bits, true);
    if (rc != RANENV_OK) return rc;
    if (!dense) return fail(h, RANENV_E_INVALID, "null sched_decision");
    rc = slice_metrics_outputs(h, obs_intra, reward);
    if (rc != RANENV_OK) return rc;
    if (!se_tiles && !h->kp.se_pool) return fail(h, RANENV_E_STATE, "a dense step reads whole SE rows: it needs explicit tiles or an RB-major pool (this handle has gather sidecars only)");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    KP kp = call_kp(h, obs_inter, obs_intra, reward, done);
    kp.se_tiles = se_tiles; kp.traffic_bits = traffic_bits; kp.dense = dense;
    h->idle_state_clean = false;                 // (a dense decision is the facade's path: explicit traffic, any UE)
    hipError_t e = launch<MODE_DENSE>(h, kp, (hipStream_t)stream);
    if (e != hipSuccess) return fail(h, RANENV_E_HIP, "dense step launch: %s", hipGetErrorString(e));
    shadow_steps_add(h, 0, h->cfg.batch, 1, done, (hipStream_t)stream);
    return RANENV_OK;
}

int ranenv_step_range(ranenv_handle h, int32_t env_first, int32_t env_count, const double *scores, const uint8_t *intra,
                      const double *traffic_bits, const float *se_tiles, float *obs_inter, float *obs_intra, double *reward,
                      uint8_t *done, void *stream)
{
    KP kp;
    hipError_t e;
    const int rc = step_begin(h, env_first, env_count, scores, intra, traffic_bits, se_tiles, obs_inter, obs_intra, reward, done,
                              (hipStream_t)stream, &kp, &e);
    if (rc != RANENV_OK) return rc;
    if (e == hipSuccess) e = launch_range<MODE_STEP>(h, kp, env_first, env_count, (hipStream_t)stream);
    if (e == hipSuccess && (h->cfg.flags & RANENV_F_SYNC_CHECK)) e = hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess) return fail(h, RANENV_E_HIP, "step launch (envs [%d,%d)): %s", env_first, env_first + env_count, hipGetErrorString(e));
    shadow_steps_add(h, env_first, env_first + env_count, 1, done, (hipStream_t)stream);
    return RANENV_OK;
}

int ranenv_step_part(ranenv_handle h, int32_t part, const double *scores, const uint8_t *intra, const double *traffic_bits,
                     const float *se_tiles, float *obs_inter, float *obs_intra, double *reward, uint8_t *done, void *stream_)
{
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    int rc = check_part(h, part);
    if (rc != RANENV_OK) return rc;
    hipStream_t ps = h->part_stream[(size_t)part];
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    rc = part_handoff(h, part, (hipStream_t)stream_);
    if (rc != RANENV_OK) return rc;
    rc = ranenv_step_range(h, h->part_lo[(size_t)part], h->part_lo[(size_t)part + 1] - h->part_lo[(size_t)part], scores, intra,
                           traffic_bits, se_tiles, obs_inter, obs_intra, reward, done, ps);
    if (rc != RANENV_OK) return rc;
    // ... and leaves an event for ranenv_wait_part
    HIP_TRY(h, hipEventRecord(h->part_done[(size_t)part], ps));
    return RANENV_OK;
}

int ranenv_wait_part(ranenv_handle h, int32_t part, void *stream_)
{
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    const int rc = check_part(h, part);
    if (rc != RANENV_OK) return rc;
    if ((hipStream_t)stream_ != h->part_stream[(size_t)part])
        HIP_TRY(h, hipStreamWaitEvent((hipStream_t)stream_, h->part_done[(size_t)part], 0));
    return RANENV_OK;
}

int ranenv_get_part_stream(ranenv_handle h, int32_t part, void **stream)
{
    if (!h || !stream) return fail(h, RANENV_E_INVALID, "null argument");
    const int rc = check_part(h, part);
    if (rc != RANENV_OK) return rc;
    *stream = (void *)h->part_stream[(size_t)part];
    return RANENV_OK;
}

int ranenv_get_partition(ranenv_handle h, int32_t part, int32_t *env_first, int32_t *env_count)
{
    if (!h || !env_first || !env_count) return fail(h, RANENV_E_INVALID, "null argument");
    if (h->part_lo.empty()) { if (part != 0) return fail(h, RANENV_E_INVALID, "partition %d outside [0,1)", part); *env_first = 0; *env_count = h->cfg.batch; return RANENV_OK; }
    if (part < 0 || part >= h->n_parts) return fail(h, RANENV_E_INVALID, "partition %d outside [0,%d)", part, h->n_parts);
    *env_first = h->part_lo[(size_t)part]; *env_count = h->part_lo[(size_t)part + 1] - h->part_lo[(size_t)part];
    return RANENV_OK;
}

int ranenv_set_se_mode(ranenv_handle h, int32_t mode, void *stream_)
{
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    if (mode != RANENV_SE_STREAM && mode != RANENV_SE_GATHER) return fail(h, RANENV_E_INVALID, "unknown SE mode %d", mode);
    if (mode == RANENV_SE_STREAM) {
        if (!h->kp.se_pool && h->se_mode == RANENV_SE_GATHER)
            return fail(h, RANENV_E_STATE, "this handle's sidecars came straight from power: there is no RB-major pool to stream (ranenv_bind_se_pool)");
        h->se_mode = RANENV_SE_STREAM; return RANENV_OK;
    }
    if (!h->kp.se_pool) {
        if (h->d_se_mean && h->se_tiles_n > 0) { h->se_mode = RANENV_SE_GATHER; return RANENV_OK; }      // sidecars straight from power
        return fail(h, RANENV_E_STATE, "the SE gather mode needs a bound SE pool (ranenv_bind_se_pool) or sidecars from power (ranenv_bind_se_gather_from_power)");
    }
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t stream = (hipStream_t)stream_;
    // (re)build the sidecars for the pool as it is now
    const int rc = se_sidecars_rebuild(h, (size_t)h->se_tiles_n, [&](size_t t0, size_t n) {
        launch_se_sidecar(stream, (unsigned)n, (unsigned)h->nt, h->kp.se_pool, (long long)h->kp.se_stride, (long long)t0, h->cfg.n_ues,
                          h->cfg.n_rbs, h->se_rp, h->kp.se_quad, h->d_se_mean, h->d_se_um);
    });
    if (rc != RANENV_OK) return rc;
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(h, RANENV_E_HIP, "SE sidecar launch: %s", hipGetErrorString(e));
    // The sidecars are read by launches on other streams (the partitions' own): a one-off multi-GB build that started with a
    // device synchronisation also ends with one, instead of an event every partition stream would have to wait for.
    HIP_TRY(h, hipStreamSynchronize(stream));
    h->se_mode = RANENV_SE_GATHER;
    return RANENV_OK;
}

int ranenv_bind_se_gather_from_power(ranenv_handle h, const double *dev_power, int64_t n_tiles, double tx_power_per_rb,
                                     double noise_power, void *stream_)
{
    if (!h || !dev_power) return fail(h, RANENV_E_INVALID, "null argument");
    if (n_tiles < 1) return fail(h, RANENV_E_INVALID, "n_tiles must be >= 1");
    if (!(noise_power > 0.0)) return fail(h, RANENV_E_INVALID, "noise_power must be positive");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t stream = (hipStream_t)stream_;
    const int rc = se_sidecars_rebuild(h, (size_t)n_tiles, [&](size_t t0, size_t n) {
        launch_se_sidecar_from_power(stream, (unsigned)n, (unsigned)h->nt, dev_power, (long long)t0, h->cfg.n_ues, h->cfg.n_rbs, h->se_rp,
                                     tx_power_per_rb, noise_power, h->d_se_mean, h->d_se_um);
    });
    if (rc != RANENV_OK) return rc;
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(h, RANENV_E_HIP, "SE sidecar-from-power launch: %s", hipGetErrorString(e));
    HIP_TRY(h, hipStreamSynchronize(stream));        // (read by launches on other streams; the power array may be freed by the caller now)
    h->kp.se_pool = nullptr; h->kp.se_stride = 0;    // no RB-major pool: pooled tiles exist as sidecars only
    h->ml_valid = false;                             // (... and no member-lines copy is ever built of them)
    h->se_tiles_n = n_tiles; h->se_mode = RANENV_SE_GATHER; h->se_stats_n = 0;
    h->have_episodes = false;                        // descriptors are re-validated against the new tile count
    return RANENV_OK;
}

int ranenv_get_se_sidecars(ranenv_handle h, double **dev_row_mean, float **dev_ue_major, int32_t *row_floats)
{
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    if (!h->d_se_mean) return fail(h, RANENV_E_STATE, "no SE sidecars (ranenv_set_se_mode GATHER builds them)");
    if (dev_row_mean) *dev_row_mean = h->d_se_mean;
    if (dev_ue_major) *dev_ue_major = h->d_se_um;
    if (row_floats) *row_floats = h->se_rp;
    return RANENV_OK;
}

int ranenv_build_se_stats(ranenv_handle h, void *stream_)
{
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    if (!h->kp.se_pool || h->se_tiles_n < 1)
        return fail(h, RANENV_E_STATE, "the tile statistics are built from a bound float32 SE pool (ranenv_bind_se_pool / ranenv_bind_se_pool_quad)%s",
                    h->d_se_mean && h->se_tiles_n > 0 ? ": this handle's sidecars came straight from power" : "");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t stream = (hipStream_t)stream_;
    const int U = h->cfg.n_ues;
    h->se_stats_n = 0;
    if (!h->d_se_stats || h->se_stats_cap < h->se_tiles_n) HIP_TRY(h, hipDeviceSynchronize());       // (an earlier caller may still read the old array)
    int64_t cap = h->se_stats_cap * 4 * U;
    const int rc = dev_grow(h, &h->d_se_stats, &cap, h->se_tiles_n * 4 * U, "SE tile statistics");
    h->se_stats_cap = h->d_se_stats ? cap / (4 * U) : 0;
    if (rc != RANENV_OK) return rc;
    const size_t nt = (size_t)h->se_tiles_n;
    for (size_t t0 = 0; t0 < nt; t0 += 1u << 20)
        launch_se_tile_stats(stream, (unsigned)(nt - t0 < (1u << 20) ? nt - t0 : (size_t)(1u << 20)), (unsigned)h->nt, h->kp.se_pool,
                             (long long)h->kp.se_stride, (long long)t0, U, h->cfg.n_rbs, h->kp.se_quad, h->d_se_stats);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(h, RANENV_E_HIP, "SE tile statistics launch: %s", hipGetErrorString(e));
    HIP_TRY(h, hipStreamSynchronize(stream));        // (read by ranenv_rbs_needed calls on any stream, and handed out by ranenv_get_se_stats)
    h->se_stats_n = h->se_tiles_n;
    return RANENV_OK;
}

int ranenv_get_se_stats(ranenv_handle h, double **dev_stats, int64_t *n_tiles)
{
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    if (h->se_stats_n < 1) return fail(h, RANENV_E_STATE, "no SE tile statistics for the pool bound now (ranenv_build_se_stats builds them)");
    if (dev_stats) *dev_stats = h->d_se_stats;
    if (n_tiles) *n_tiles = h->se_stats_n;
    return RANENV_OK;
}

int ranenv_rbs_needed(ranenv_handle h, const ranenv_episode *eps, int32_t n_episodes, int32_t n_steps, double *dev_slice, double *dev_network,
                      double *dev_episode_mean, void *stream_)
{
    // ---- everything is validated before the first device call ----
    if (!h || !eps || !dev_episode_mean) return fail(h, RANENV_E_INVALID, "null argument");
    if (!h->have_scenarios) return fail(h, RANENV_E_STATE, "load scenarios first");
    if (h->se_stats_n < 1) return fail(h, RANENV_E_STATE, "no SE tile statistics for the pool bound now (ranenv_build_se_stats builds them)");
    if (n_episodes < 1) return fail(h, RANENV_E_INVALID, "n_episodes must be >= 1, got %d", n_episodes);
    if (n_steps < 1) return fail(h, RANENV_E_INVALID, "n_steps must be >= 1, got %d", n_steps);
    if ((long long)n_episodes * n_steps >= (1ll << 31))
        return fail(h, RANENV_E_INVALID, "n_episodes * n_steps = %lld: one call takes fewer than 2^31 (episode, step) pairs", (long long)n_episodes * n_steps);
    for (int i = 0; i < n_episodes; i++) {
        const ranenv_episode &e = eps[i];
        if (e.scenario < 0 || e.scenario >= h->cfg.n_scenarios)
            return fail(h, RANENV_E_INVALID, "episode %d: scenario %d outside pool of %d", i, e.scenario, h->cfg.n_scenarios);
        if (e.se_len < 1 || e.se_offset < 0 || e.se_offset >= e.se_len || e.se_base < 0)
            return fail(h, RANENV_E_INVALID, "episode %d: need se_len >= 1, 0 <= se_offset < se_len, se_base >= 0", i);
        if (e.se_base + e.se_len > h->se_stats_n)
            return fail(h, RANENV_E_INVALID, "episode %d: SE trace [%lld,+%d) exceeds the pool of %lld tiles the statistics were built from", i,
                        (long long)e.se_base, e.se_len, (long long)h->se_stats_n);
    }
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t stream = (hipStream_t)stream_;
    const int S = h->cfg.n_slices, U = h->cfg.n_ues;
    int rc = dev_grow(h, &h->d_load_eps, &h->load_eps_cap, (int64_t)n_episodes, "scenario load descriptors");
    if (rc == RANENV_OK && !dev_network) rc = dev_grow(h, &h->d_load_net, &h->load_net_cap, (int64_t)n_episodes * n_steps * 3, "scenario load network rows");
    if (rc != RANENV_OK) return rc;
    HIP_TRY(h, hipMemcpyAsync(h->d_load_eps, eps, sizeof(ranenv_episode) * (size_t)n_episodes, hipMemcpyHostToDevice, stream));
    RbsArgs a;
    a.eps = h->d_load_eps; a.n_steps = n_steps; a.stats = h->d_se_stats;
    a.ue_slice = h->kp.tab.ue + (size_t)6 * (size_t)h->kp.NSU;      // set 1 of the per-UE tables: entry u = UE u (ranenv_internal.h, Tables::ue)
    a.slice_i32 = h->kp.tab.slice_i32; a.slice_f64 = h->kp.tab.slice_f64;
    a.S = S; a.U = U; a.R = h->cfg.n_rbs; a.bw_mhz = h->cfg.bandwidth_hz / 1e6;
    a.slice_out = dev_slice; a.net_out = dev_network ? dev_network : h->d_load_net;
    const int lanes = 6 * S > h->nt ? 6 * S : h->nt;                // one thread per UE, and 6 per slice for the sums
    launch_rbs_needed(stream, (unsigned)n_episodes, (unsigned)((lanes + WAVE - 1) / WAVE * WAVE), a, dev_episode_mean);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(h, RANENV_E_HIP, "scenario load launch: %s", hipGetErrorString(e));
    HIP_TRY(h, hipStreamSynchronize(stream));        // the staging buffers are the handle's: free for the next call
    return RANENV_OK;
}

int ranenv_profile_begin(ranenv_handle h)
{
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    h->prof_used = 0; h->prof_ttis = 0; h->prof_env_ttis = 0; h->prof_on = true;
    return RANENV_OK;
}

int ranenv_profile_ttis(ranenv_handle h, int64_t *n_ttis)
{
    if (!h || !n_ttis) return fail(h, RANENV_E_INVALID, "null argument");
    *n_ttis = (int64_t)h->prof_ttis;
    return RANENV_OK;
}

int ranenv_profile_work(ranenv_handle h, int64_t *n_ttis, int64_t *n_env_ttis)
{
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    if (n_ttis) *n_ttis = (int64_t)h->prof_ttis;
    if (n_env_ttis) *n_env_ttis = (int64_t)h->prof_env_ttis;
    return RANENV_OK;
}

int ranenv_profile_end(ranenv_handle h, double *avg_ms, int32_t *n_launches)
{
    if (!h || !avg_ms || !n_launches) return fail(h, RANENV_E_INVALID, "null argument");
    if (!h->prof_on) return fail(h, RANENV_E_STATE, "ranenv_profile_begin was not called");
    h->prof_on = false;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipDeviceSynchronize());
    double acc = 0.0;
    for (size_t i = 0; i + 1 < h->prof_used; i += 2) {
        float ms = 0.0f;
        HIP_TRY(h, hipEventElapsedTime(&ms, h->prof_ev[i], h->prof_ev[i + 1]));
        acc += (double)ms;
    }
    *n_launches = (int32_t)(h->prof_used / 2);
    *avg_ms = h->prof_used ? acc / (double)(h->prof_used / 2) : 0.0;
    return RANENV_OK;
}

int ranenv_set_partitions(ranenv_handle h, int32_t n_parts)
{
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    if (n_parts < 1 || n_parts > 16 || n_parts > h->cfg.batch) return fail(h, RANENV_E_INVALID, "n_parts must be in [1, min(16, batch)]");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipDeviceSynchronize());
    HIP_TRY(h, ensure_streams(h, (size_t)n_parts));
    h->part_lo.assign((size_t)n_parts + 1, 0);
    // (an even batch is cut into even ranges where that is possible: packed waves step two envs each, ranenv_core_kernel_packed)
    const int B = h->cfg.batch, unit = (B % 2 == 0 && B / 2 >= n_parts) ? 2 : 1;
    const int base = (B / unit) / n_parts, rem = (B / unit) % n_parts;
    for (int k = 0; k < n_parts; k++) h->part_lo[k + 1] = h->part_lo[k] + unit * (base + (k < rem ? 1 : 0));
    h->n_parts = n_parts;
    return RANENV_OK;
}

// ---- ranenv_rollout ---------------------------------------------------------------------------------------------------------------
// What its two schedules share.  With auto-reset on, an env whose episode ends inside the rollout moves on to its next episode
// without the host: the advance kernel + the step kernel in RESET mode follow that TTI's step on the partition's stream.  They are
// only enqueued for TTIs at which some env of the partition finishes: the step counters are read once at the start and followed on
// the host (nothing but this rollout changes them until it returns).
// What a rollout records beside stepping.  ranenv_collect / ranenv_collect_head: the caller's record, from either public struct
struct Record {
    PolicyRec rec{};               // slot 0 of what the policy launches write (head: obs_inter / action_inter are its obs_head / action, cols = 1)
    int gae_col = 0;               // GAE(gamma, lambda) runs on rec.cols columns of the reward rows from column gae_col on
    double gamma = 0.0, lambda = 0.0;
    float *adv = nullptr, *vtarg = nullptr;
};
// ... or ranenv_collect_replay's ring; and, either way, where the step writes a TTI's done flags and reward rows (under a head policy
// with source HEAD: the head kernel its reward pairs) instead of the caller's buffers: slot (first + t) % slots of [slots][B] / [slots][B][reward_cols]
struct Recording {
    const Record *ppo = nullptr;
    const ranenv_replay *ring = nullptr;
    uint8_t *done = nullptr; double *reward = nullptr;      // (null: not recorded)
    int reward_cols = 0;
    long long first = 0, slots = 1;
    size_t slot(int t) const { return (size_t)((first + t) % slots); }
};

struct Rollout {
    int n_steps = 0;
    KP kp{};                       // the step's
    int net = 0;                   // the policy nets run in front of every TTI
    bool follow = false;           // auto-reset on: the host's copy of the step counters, the advance kernel's arguments, the reset's KP
    std::vector<int32_t> steps;
    AdvanceArgs adv{};
    KP kpr{};
    const Recording *rec = nullptr;      // (null: a plain rollout)
};

// TTIs from now until the first episode of envs [lo, hi) ends, that TTI included, between 1 and n.  `n_ends`: at how many different
// TTIs before the n-th episodes end (counted up to 3).
static int ttis_to_end(const ranenv *h, const Rollout &r, int lo, int hi, int n, int *n_ends = nullptr)
{
    int first = n, ends[3], k = 0;
    for (int b = lo; b < hi; b++) {
        const int d = max_steps_of_env(h, b) - r.steps[(size_t)b];
        if (d < first) first = d;
        if (n_ends && d < n && k < 3 && std::find(ends, ends + k, d) == ends + k) ends[k++] = d;
    }
    if (n_ends) *n_ends = k;
    return first < 1 ? 1 : first;
}

// n_tti TTIs of envs [e0, e0 + n) were enqueued on `s`: the host's step counters advance by n_tti, and the envs whose episode
// ended restart, on the host and -- advance kernel, reset -- on `s`
static hipError_t follow_episode_ends(ranenv_handle h, Rollout &r, int e0, int n, int n_tti, hipStream_t s, const uint8_t *done = nullptr)
{
    if (!r.follow) return hipSuccess;
    bool any = false;
    for (int b = e0; b < e0 + n; b++) {
        r.steps[(size_t)b] += n_tti;
        if (r.steps[(size_t)b] >= max_steps_of_env(h, b)) { any = true; r.steps[(size_t)b] = 0; }
    }
    if (!any) return hipSuccess;
    AdvanceArgs a = r.adv; a.e0 = e0;
    if (done) a.done = done;                       // (a recording rollout: the step wrote the flags into the slot)
    h->pclass_dirty = true;                        // the restarted envs' scenarios
    launch_advance(s, (unsigned)n, a);
    return launch_range<MODE_RESET>(h, r.kpr, e0, n, s);
}

// Option "persist": one persistent work-queue launch per workgroup class for all the TTIs up to the next episode end
// (ranenv_persist_kernel), on the caller's stream (+ one handle-owned stream per further class), whatever the partitions.
static int rollout_persistent(ranenv_handle h, Rollout &r, hipStream_t stream)
{
    h->last_rollout_persistent = 1;
    for (int done_ttis = 0; done_ttis < r.n_steps;) {
        int n_tti = r.n_steps - done_ttis;
        if (r.follow) n_tti = ttis_to_end(h, r, 0, h->cfg.batch, n_tti);
        if (n_tti >= (1 << (31 - PERSIST_ENV_BITS))) n_tti = (1 << (31 - PERSIST_ENV_BITS)) - 1;
        int rc = persist_prepare(h, stream, true);
        if (rc != RANENV_OK) return rc;
        rc = persist_launch(h, r.kp, n_tti, stream);
        if (rc != RANENV_OK) return rc;
        done_ttis += n_tti;
        const hipError_t re = follow_episode_ends(h, r, 0, h->cfg.batch, n_tti, stream);
        if (re != hipSuccess) return fail(h, RANENV_E_HIP, "persistent rollout, reset launch: %s", hipGetErrorString(re));
    }
    return RANENV_OK;
}

constexpr long long COLLECT_FUSED_MAX_BYTES = 3ll << 20;      // actor + critic weights that share an XCD's 4 MB of L2 with the activations' traffic

// a: the actor's slot, v: its critic's (null: none runs) -- each counts with one copy (slot_copy_floats)
static int collect_split_of(ranenv_handle h, const ranenv::NetSlot &a, const ranenv::NetSlot *v)
{
    if (!v) return 0;
    if (h->collect_split >= 0) return h->collect_split;
    return (slot_copy_floats(a) + slot_copy_floats(*v)) * (long long)sizeof(float) > COLLECT_FUSED_MAX_BYTES ? 1 : 0;
}

// ranenv_collect / ranenv_collect_head: the recording policy launches (actors, record, critics) of envs [e0, e0 + n) on `s` into slot t of
// the record, or -- critic_only -- the critics alone on the observation as it stands: vf[t]
static hipError_t collect_policy(ranenv_handle h, const Record &tr, const KP &kpk, int t, bool critic_only, int e0, int n, hipStream_t s)
{
    const bool head = head_policy(h);
    const size_t B = (size_t)h->cfg.batch, S = (size_t)h->cfg.n_slices, Us = (size_t)h->cfg.max_ues_slice, W = 2 * Us + 9, C = (size_t)tr.rec.cols;
    const bool ia = !head && h->serving_net(NET_INTRA), vc = tr.rec.vf != nullptr, ic = vc && !head && h->serving_net(NET_INTRA_VALUE);
    auto slot = [&](auto *p, size_t stride) { return p ? p + (size_t)t * B * stride : nullptr; };
    PolicyRec rec{};
    rec.vf = slot(tr.rec.vf, C);
    rec.cols = (int)C; rec.intra_critic = ic ? 1 : 0; rec.critic_only = critic_only ? 1 : 0;
    if (!critic_only) {
        rec.obs_inter = slot(tr.rec.obs_inter, 10 * S);
        rec.mask_inter = slot(tr.rec.mask_inter, S);
        rec.action_inter = slot(tr.rec.action_inter, S);
        if (ia) {
            rec.obs_intra = slot(tr.rec.obs_intra, S * W);
            rec.mask_intra = slot(tr.rec.mask_intra, S * Us);
            rec.action_intra = slot(tr.rec.action_intra, S);
        }
        rec.logp = slot(tr.rec.logp, C);
        rec.intra_actor = ia ? 1 : 0;
    }
    PolicyNets nets = head ? PolicyNets{true, &h->head.net, nullptr, vc ? &h->head_value.net : nullptr, nullptr} : h->ibsched_nets(vc);
    // Actor and critic in one launch share the L2 of their XCD (4 MB): fused where both weight sets fit in it together, else the
    // critic runs as a launch of its own behind the actor's, each with the L2 to itself (measured, DESIGN.md 4.p "Collection").  Nets per
    // slice count with one slice's copy: the co-resident workgroups of a sliced launch mostly walk one slice's weights.
    if (!critic_only)
        rec.split = head ? collect_split_of(h, h->head, vc ? &h->head_value : nullptr)
                         : collect_split_of(h, *h->serving(NET_INTER), vc ? h->serving(NET_INTER_VALUE) : nullptr) |
                               (ia ? collect_split_of(h, *h->serving(NET_INTRA), ic ? h->serving(NET_INTRA_VALUE) : nullptr) << 1 : 0);
    return launch_policy(s, nets, net_io(h, kpk), &rec, e0, n);
}

// One launch of a partition's walk: TTI `t` of its own count, kpk.n_tti TTIs (one under a policy net or a recording), for envs
// [e0, e0 + n) on `s`.  The order on the stream is the content of two rules.  The ring's next_obs is copied BEFORE the reset behind an
// episode end refreshes the head observation: the terminal observation of the envs that finished, the next slot's obs of all others.
// The record's vf[T] is computed BEHIND that reset: the value of the observation the next call starts from.
static hipError_t rollout_tti(ranenv_handle h, Rollout &r, KP kpk, int t, int e0, int n, hipStream_t s)
{
    const Recording *rec = r.rec;
    const Record *ppo = rec ? rec->ppo : nullptr;
    const ranenv_replay *ring = rec ? rec->ring : nullptr;
    const size_t B = (size_t)h->cfg.batch, S = (size_t)h->cfg.n_slices, row = rec ? rec->slot(t) * B : 0;      // the slot's first row
    // 1. the policy: recording (actors, record, critics), plain, or none
    hipError_t le = ppo ? collect_policy(h, *ppo, kpk, t, false, e0, n, s) : (r.net ? net_launch(h, kpk, e0, n, s) : hipSuccess);
    if (le != hipSuccess) return le;
    // 2. the step's done flags and reward rows go straight into the slot (the kernels index them by env; the reset writes neither, reset_behind)
    if (rec && rec->reward) (head_policy(h) && !head_inter(h) ? kpk.head_reward : kpk.reward) = rec->reward + row * (size_t)rec->reward_cols;
    if (rec && rec->done) kpk.done = rec->done + row;
    // 3. ring: the partition's rows -- one contiguous range of the slot -- of the observation the action was computed from and of the scores
    // the step consumes (one launch for both: the actor only read the observation)
    typedef unsigned long long word;
    const size_t at = row + (size_t)e0;
    const long long obs_words = (long long)n * 5 * (long long)S;      // a row: 10 * S floats
    const word *head_rows = ring ? (const word *)((head_inter(h) ? kpk.obs_inter : h->kp.head_obs) + (size_t)e0 * 10 * S) : nullptr;
    if (ring)
        launch_copy_words(s, (word *)(ring->obs + at * 10 * S), head_rows, obs_words, (word *)(ring->action + at * S),
                          (const word *)(h->d_net_scores + (size_t)e0 * S), (long long)n * (long long)S);
    // 4. the step;  5. ring: the observation the head kernel (source INTER: the step) left;  6. the episode ends, by the slot's flags
    le = launch_range<MODE_STEP>(h, kpk, e0, n, s);
    if (le != hipSuccess) return le;
    if (ring) launch_copy_words(s, (word *)(ring->next_obs + at * 10 * S), head_rows, obs_words, nullptr, nullptr, 0);
    le = follow_episode_ends(h, r, e0, n, kpk.n_tti, s, kpk.done);
    // 7. record, behind the call's last TTI: the critics once more
    if (le != hipSuccess || !ppo || !ppo->rec.vf || t + 1 < r.n_steps) return le;
    return collect_policy(h, *ppo, kpk, t + 1, true, e0, n, s);
}

// THE PLAN of a rollout: one persistent work-queue launch per class (rollout_persistent) or launches per chunk of at most `fuse` TTIs
// (rollout_chunks), and whether those launches would read the member-lines copy.  Made once per call from the handle, the call's Rollout
// -- compact steps decided, the step counters read back -- and whether the stream is capturing: no HIP call, nothing written.
struct RolloutPlan { bool persistent; int fuse; bool member_lines; };
// Auto persistent where it was measured to win or tie (profiles/r04_ab_log.txt, r05_ab_log.txt, r06_ab_log.txt): either mode
// at <= 2 waves per SIMD (persist_tiny), SE gather mode up to ~2x what the chip holds (beyond, every chunk swaps envs), and streaming
// rollouts of 4...64 TTIs at <= 20 envs per CU (the streaming kernel is bound by HBM either way: larger batches and longer rollouts tie or lose)
constexpr long long PERSIST_GATHER_MAX_ENVS_PER_CU = 44, PERSIST_STREAM_MAX_ENVS_PER_CU = 20, PERSIST_STREAM_MIN_TTIS = 4, PERSIST_STREAM_MAX_TTIS = 64;
// ... but not when episodes end at more than two different TTIs inside the call (per-env episode lengths, envs reset at different times): every
// end stops the persistent launches, re-sorts the envs and reads the class counts back; launches per chunk follow the ends per partition without a host sync
constexpr int PERSIST_MAX_EPISODE_ENDS = 2;
// A launch per chunk takes its envs through several TTIs where nothing has to happen in between (see step_loop; with auto-reset: no episode
// end before its last TTI): a quarter of the rollout, at most 10 (measured, profiles/r03_ab_log.txt: longer launches gain nothing more
// and lengthen the drain at the rollout's end, where the workgroups that waited for a free slot run last and alone)
constexpr int FUSE_ROLLOUT_PART = 4, FUSE_MAX_TTIS = 10;
static RolloutPlan rollout_plan(const ranenv *h, const Rollout &r, bool capturing)
{
    const int k = r.n_steps;
    const long long B = h->cfg.batch, N = h->n_cus;
    const bool gather = h->se_mode == RANENV_SE_GATHER;
    // ONE TTI PER LAUNCH where something runs between two TTIs: the policy nets in front of every step, the head, slice-metrics or trace kernel behind it
    const bool one_tti = r.kp.head_obs || r.kp.head_reward || r.net || slice_metrics_on(h) || trace_on(h);
    RolloutPlan p{false, one_tti ? 1 : (h->fuse > 0 ? h->fuse : std::clamp(k / FUSE_ROLLOUT_PART, 1, FUSE_MAX_TTIS)), false};
    const bool wins = persist_tiny(h) || (!h->small_batch && (gather ? B <= PERSIST_GATHER_MAX_ENVS_PER_CU * N
                          : B <= PERSIST_STREAM_MAX_ENVS_PER_CU * N && k >= PERSIST_STREAM_MIN_TTIS && k <= PERSIST_STREAM_MAX_TTIS));
    p.persistent = (RANENV_DIAG == 0 || RANENV_DIAG == 12 || RANENV_DIAG == 13) && (h->persist == 1 || (h->persist < 0 && wins)) && !one_tti && !scale_per_element(h) &&
                   r.kp.compact != 0 && (B >> PERSIST_ENV_BITS) == 0 && !capturing;      // (its classes are those of the compact lane order; it reads the class counts back)
    int n_ends = 0;
    if (p.persistent && h->persist < 0 && r.follow) (void)ttis_to_end(h, r, 0, h->cfg.batch, k, &n_ends);
    p.persistent = p.persistent && n_ends <= PERSIST_MAX_EPISODE_ENDS;
    // Member lines (option "member_lines"; auto = on): wanted where the build of the persistent launches, or of the first partition's
    // launches of several TTIs, reads an offered copy (persist_choice, step_choice: compact streaming rollouts)
    const StepFacts chunk{MODE_STEP, 2, r.kp.compact, gather, 0, h->n_parts > 1 ? h->part_lo[1] : h->cfg.batch, true};
    p.member_lines = h->member_lines != 0 && h->kp.se_pool != nullptr &&
                     (p.persistent ? persist_choice(h, true).members : k > 1 && p.fuse > 1 && step_choice(h, chunk).l.members);
    return p;
}

// Every partition walks through the TTIs in launches of its own, on its own stream, of at most `fuse` TTIs
static int rollout_chunks(ranenv_handle h, Rollout &r, int fuse, hipStream_t stream)
{
    const int n_steps = r.n_steps;
    // `pdone[k]` TTIs are enqueued for partition k
    const int np = h->n_parts > 1 ? h->n_parts : 1;
    std::vector<int> pdone((size_t)np, 0), pn((size_t)np, 0);
    auto part_of = [&](int e0) { for (int k = 0; k < np; k++) if (np > 1 && h->part_lo[k] == e0) return k; return 0; };
    for (int round = 0;; round++) {
        bool any_left = false, last = true;
        for (int k = 0; k < np; k++) {
            const int left = n_steps - pdone[(size_t)k];
            int n_tti = left < fuse ? left : fuse;
            if (round == 0 && fuse > 1 && np > 1) {
                // The partitions' first launches differ in length, the one enqueued last (the highest partition) starting with a
                // single TTI: its workgroups are the ones that find the slots taken, and after one short launch its late starters are
                // through instead of holding its chain up for a whole long one; from then on the partitions' launch boundaries no
                // longer coincide (profiles/r03_ab_log.txt).  RANENV_FUSE_FIRST=a,b,c overrides (0 = the common length).
                int first = k == np - 1 ? 1 : ((k & 1) ? (3 * fuse + 4) / 5 : fuse);
                if (!h->fuse_first.empty()) first = (size_t)k < h->fuse_first.size() ? h->fuse_first[(size_t)k] : 0;
                if (first > 0 && first < n_tti) n_tti = first;
            }
            if (r.follow && n_tti > 1)
                n_tti = ttis_to_end(h, r, np > 1 ? h->part_lo[k] : 0, np > 1 ? h->part_lo[k + 1] : h->cfg.batch, n_tti);
            pn[(size_t)k] = n_tti > 0 ? n_tti : 0;
            if (pn[(size_t)k] > 0) any_left = true;
            if (pdone[(size_t)k] + pn[(size_t)k] < n_steps) last = false;
        }
        if (!any_left) break;
        const hipError_t e = for_partitions(h, stream, round == 0, last, [&](int e0, int n, hipStream_t s) -> hipError_t {
            const int n_tti = pn[(size_t)part_of(e0)];
            if (n_tti == 0) return hipSuccess;                                    // this partition is through
            KP kpk = r.kp;
            kpk.n_tti = n_tti;
            h->last_rollout_launches++;
            return rollout_tti(h, r, kpk, pdone[(size_t)part_of(e0)], e0, n, s);
        });
        if (e != hipSuccess) return fail(h, RANENV_E_HIP, "rollout, round %d of launches: %s", round, hipGetErrorString(e));
        for (int k = 0; k < np; k++) pdone[(size_t)k] += pn[(size_t)k];
    }
    return RANENV_OK;
}

// ranenv_rollout, and with `rec` ranenv_collect / ranenv_collect_head / ranenv_collect_replay
static int rollout_run(ranenv_handle h, int32_t n_steps, float *obs_inter, float *obs_intra, double *reward, uint8_t *done, void *stream_,
                       const Recording *rec = nullptr)
{
    int rc = check_ready(h, nullptr, nullptr, true);
    if (rc != RANENV_OK) return rc;
    if (n_steps < 1) return fail(h, RANENV_E_INVALID, "n_steps must be >= 1");
    rc = slice_metrics_outputs(h, obs_intra, reward);
    if (rc != RANENV_OK) return rc;
    rc = trace_outputs(h, nullptr, obs_inter, obs_intra, reward, done);
    if (rc != RANENV_OK) return rc;
    if (h->kp.policy == RANENV_POLICY_EXTERNAL) return fail(h, RANENV_E_STATE, "a rollout needs a device policy (ranenv_set_policy MARR / MAPF / NETWORK)");
    if (head_inter(h) && h->head.on && !obs_inter) return fail(h, RANENV_E_INVALID, "the policy network reads obs_inter: the step needs that buffer");
    const bool have_se = h->kp.se_pool != nullptr || (h->se_mode == RANENV_SE_GATHER && h->d_se_mean != nullptr);
    if (!have_se || (!h->kp.trf_pool && !h->kp.trf_gen)) return fail(h, RANENV_E_STATE, "a rollout replays the bound SE pool and traffic pool / generator");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    rc = persist_check_errors(h);                  // (of the persistent launches of earlier calls that have completed)
    if (rc != RANENV_OK) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    Rollout r;
    r.n_steps = n_steps;
    r.kp = call_kp(h, obs_inter, obs_intra, reward, done);
    h->last_rollout_persistent = 0; h->last_rollout_launches = 0; h->last_rollout_member_lines = 0; h->last_rollout_lean_ttis = 0; h->last_rollout_kept_state_ttis = 0;
    r.net = net_use(h, r.kp);                      // (policy network: its launch precedes every TTI of a partition, see rollout_plan)
    if (r.net < 0) return r.net;
    r.rec = rec;
    rc = compact_for(h, r.kp, stream, &r.kp.compact);
    if (rc != RANENV_OK) return rc;
    if (r.kp.compact) r.kp.compact = 2;             // (2: the streaming kernels may step compactly too, see step_choice)
    r.follow = h->ar_on;
    if (r.follow) {
        if (!done) return fail(h, RANENV_E_INVALID, "a rollout with auto-reset needs the done buffer");
        std::vector<int32_t> &steps = r.steps;
        steps.resize((size_t)h->cfg.batch);
        HIP_TRY(h, hipStreamSynchronize(stream));
        HIP_TRY(h, hipMemcpy(steps.data(), ST_step_no(h->kp), sizeof(int32_t) * steps.size(), hipMemcpyDeviceToHost));
        r.adv = advance_args(h, done, obs_inter, obs_intra, nullptr, nullptr, nullptr);
        r.kpr = reset_behind(h, r.kp);
    }
    const RolloutPlan plan = rollout_plan(h, r, stream_capturing(stream));
    // (the handle's per-UE line copy of the pool is built by the first rollout that would use it, never inside a stream capture: member_lines_ready)
    if (plan.member_lines && member_lines_ready(h, stream)) { r.kp.ml_pool = h->d_ml; r.kp.ml_stride = h->ml_stride; }
    rc = plan.persistent ? rollout_persistent(h, r, stream) : rollout_chunks(h, r, plan.fuse, stream);
    if (rc != RANENV_OK) return rc;
    if (rec) {
        // (the partitions have joined the caller's stream)  The caller's reward -- under a head policy with source HEAD: the bound head rewards -- and
        // done hold the last TTI's values, as after a rollout
        const size_t B = (size_t)h->cfg.batch, C = (size_t)rec->reward_cols, last = rec->slot(n_steps - 1) * B;
        double *last_reward = head_policy(h) && !head_inter(h) ? h->kp.head_reward : reward;
        if (rec->reward && last_reward)
            HIP_TRY(h, hipMemcpyAsync(last_reward, rec->reward + last * C, sizeof(double) * B * C, hipMemcpyDeviceToDevice, stream));
        if (rec->done && done) HIP_TRY(h, hipMemcpyAsync(done, rec->done + last, B, hipMemcpyDeviceToDevice, stream));
        if (const Record *ppo = rec->ppo; ppo && (ppo->adv || ppo->vtarg)) {
            if (h->gae_on && !head_policy(h)) {      // ranenv_set_population_gae: member m's pair for member m's envs
                GaePop g{};
                g.pop = h->pop;
                for (int m = 0; m < h->pop.n; m++) { g.gamma[m] = h->gae_gamma[m]; g.lambda[m] = h->gae_lambda[m]; }
                launch_gae_pop(stream, n_steps, h->cfg.batch, ppo->rec.cols, rec->reward + ppo->gae_col, (int)C, ppo->rec.vf, rec->done, g, ppo->adv, ppo->vtarg);
            } else
            launch_gae(stream, n_steps, h->cfg.batch, ppo->rec.cols, rec->reward + ppo->gae_col, (int)C, ppo->rec.vf, rec->done, ppo->gamma,
                       ppo->lambda, ppo->adv, ppo->vtarg);
            HIP_TRY(h, hipGetLastError());
        }
        if (rec->ring) h->ring_written += n_steps;
    }
    if (r.follow) { h->sh_steps = r.steps; h->sh_valid = true; h->last_done = done; }      // (read from the device above, followed exactly since)
    else shadow_steps_add(h, 0, h->cfg.batch, n_steps, done, stream);
    return RANENV_OK;
}

int ranenv_rollout(ranenv_handle h, int32_t n_steps, float *obs_inter, float *obs_intra, double *reward, uint8_t *done, void *stream)
{
    return rollout_run(h, n_steps, obs_inter, obs_intra, reward, done, stream);
}

static_assert(sizeof(ranenv_trajectory) == RANENV_TRAJECTORY_BYTES, "ranenv_trajectory: 12 device pointers");

int ranenv_collect(ranenv_handle h, int32_t n_steps, const ranenv_trajectory *traj, double gamma, double lambda, float *obs_inter,
                   float *obs_intra, double *reward, uint8_t *done, void *stream)
{
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    if (!traj) return fail(h, RANENV_E_INVALID, "null trajectory");
    if (n_steps < 1) return fail(h, RANENV_E_INVALID, "n_steps must be >= 1");
    if ((traj->adv || traj->vtarg) && !(traj->reward && traj->vf && traj->done))
        return fail(h, RANENV_E_INVALID, "adv / vtarg need the record's reward, vf and done");
    if (h->kp.policy != RANENV_POLICY_NETWORK) return fail(h, RANENV_E_STATE, "ranenv_collect needs policy NETWORK (ranenv_set_policy)");
    if (!h->serving(NET_INTER)) return fail(h, RANENV_E_STATE, "policy NETWORK but no policy network bound (ranenv_set_policy_network)");
    if (!h->serving(NET_INTER_VALUE)) return fail(h, RANENV_E_STATE, "no value network bound (ranenv_set_value_network)");
    if (h->serving_net(NET_INTRA_VALUE) && !(h->serving_net(NET_INTRA) && h->serving_net(NET_INTRA)->layout == h->serving_net(NET_INTRA_VALUE)->layout))
        return fail(h, RANENV_E_STATE, "the intra value net was bound for another intra policy net (bind it again, ranenv_set_value_network)");
    Record ppo;
    ppo.rec.obs_inter = traj->obs_inter; ppo.rec.obs_intra = traj->obs_intra; ppo.rec.mask_inter = traj->mask_inter; ppo.rec.mask_intra = traj->mask_intra;
    ppo.rec.action_inter = traj->action_inter; ppo.rec.action_intra = traj->action_intra; ppo.rec.logp = traj->logp; ppo.rec.vf = traj->vf;
    ppo.rec.cols = h->cfg.n_slices + 1;
    ppo.gamma = gamma; ppo.lambda = lambda; ppo.adv = traj->adv; ppo.vtarg = traj->vtarg;
    const Recording rec{&ppo, nullptr, traj->done, traj->reward, ppo.rec.cols, 0, n_steps};
    return rollout_run(h, n_steps, obs_inter, obs_intra, reward, done, stream, &rec);
}

static_assert(sizeof(ranenv_head_trajectory) == RANENV_HEAD_TRAJECTORY_BYTES, "ranenv_head_trajectory: 8 device pointers");

// ranenv_collect_head / ranenv_replay_sample: the column of the recorded reward rows, by the head policy source
static int head_reward_col_check(ranenv_handle h, int32_t reward_col)
{
    if (h->head_src == RANENV_HEAD_SRC_INTER) {
        if (reward_col < 0 || reward_col > h->cfg.n_slices)
            return fail(h, RANENV_E_INVALID, "reward_col %d (source INTER: 0 = player_0 .. %d of the step's reward row)", reward_col, h->cfg.n_slices);
        return RANENV_OK;
    }
    if (reward_col != 0 && reward_col != 1) return fail(h, RANENV_E_INVALID, "reward_col %d (0 = SchedTWC, 1 = SchedColORAN)", reward_col);
    return RANENV_OK;
}

int ranenv_collect_head(ranenv_handle h, int32_t n_steps, const ranenv_head_trajectory *traj, int32_t reward_col, double gamma, double lambda,
                        float *obs_inter, float *obs_intra, double *reward, uint8_t *done, void *stream)
{
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    if (!traj) return fail(h, RANENV_E_INVALID, "null trajectory");
    if (n_steps < 1) return fail(h, RANENV_E_INVALID, "n_steps must be >= 1");
    if (const int rc = head_reward_col_check(h, reward_col); rc != RANENV_OK) return rc;
    if ((traj->adv || traj->vtarg) && !(traj->reward_head && traj->vf && traj->done))
        return fail(h, RANENV_E_INVALID, "adv / vtarg need the record's reward_head, vf and done");
    if (h->kp.policy != RANENV_POLICY_HEAD_NETWORK) return fail(h, RANENV_E_STATE, "ranenv_collect_head needs policy HEAD_NETWORK (ranenv_set_policy)");
    if (!h->head.on) return fail(h, RANENV_E_STATE, "policy HEAD_NETWORK but no head policy network bound (ranenv_set_head_policy_network)");
    if (h->head_dist != RANENV_HEAD_DIST_GAUSS_CLIP)
        return fail(h, RANENV_E_INVALID, "only GAUSS_CLIP (PPO) head policies collect: SAC is off-policy and records no log-probabilities");
    if (!h->head_value.on) return fail(h, RANENV_E_STATE, "no head value network bound (ranenv_set_head_value_network)");
    Record ppo;
    ppo.rec.obs_inter = traj->obs_head; ppo.rec.action_inter = traj->action; ppo.rec.logp = traj->logp; ppo.rec.vf = traj->vf;
    ppo.rec.cols = 1; ppo.gae_col = reward_col;
    ppo.gamma = gamma; ppo.lambda = lambda; ppo.adv = traj->adv; ppo.vtarg = traj->vtarg;
    const Recording rec{&ppo, nullptr, traj->done, traj->reward_head, head_reward_cols(h), 0, n_steps};
    return rollout_run(h, n_steps, obs_inter, obs_intra, reward, done, stream, &rec);
}

// ---- off-policy collection (SAC): replay ring, sampler, targets -------------------------------------------------------------------
static_assert(sizeof(ranenv_replay) == RANENV_REPLAY_BYTES, "ranenv_replay: two int32 and 5 device pointers");

static bool aligned8(const void *p) { return ((uintptr_t)p & 7) == 0; }

int ranenv_bind_replay(ranenv_handle h, const ranenv_replay *ring)
{
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    if (!ring) { h->ring = ranenv_replay{}; h->ring_on = false; h->ring_written = 0; return RANENV_OK; }
    if (ring->capacity < 2) return fail(h, RANENV_E_INVALID, "replay ring: capacity %d (>= 2 slots)", ring->capacity);
    if (!ring->obs || !ring->next_obs || !ring->action || !ring->reward_head || !ring->done)
        return fail(h, RANENV_E_INVALID, "replay ring: obs, next_obs, action, reward_head and done are all required");
    if (!aligned8(ring->obs) || !aligned8(ring->next_obs) || !aligned8(ring->action) || !aligned8(ring->reward_head))
        return fail(h, RANENV_E_INVALID, "replay ring: the arrays must be 8-byte aligned");
    h->ring = *ring; h->ring_on = true; h->ring_written = 0;
    return RANENV_OK;
}

int ranenv_get_replay_count(ranenv_handle h, int64_t *written)
{
    if (!h || !written) return fail(h, RANENV_E_INVALID, "null argument");
    *written = h->ring_on ? h->ring_written : 0;
    return RANENV_OK;
}

int ranenv_collect_replay(ranenv_handle h, int32_t n_steps, float *obs_inter, float *obs_intra, double *reward, uint8_t *done, void *stream)
{
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    if (n_steps < 1) return fail(h, RANENV_E_INVALID, "n_steps must be >= 1");
    if (!h->ring_on) return fail(h, RANENV_E_STATE, "no replay ring bound (ranenv_bind_replay)");
    if (n_steps > h->ring.capacity) return fail(h, RANENV_E_INVALID, "n_steps %d exceeds the ring's capacity %d", n_steps, h->ring.capacity);
    if (h->kp.policy != RANENV_POLICY_HEAD_NETWORK) return fail(h, RANENV_E_STATE, "ranenv_collect_replay needs policy HEAD_NETWORK (ranenv_set_policy)");
    if (!h->head.on) return fail(h, RANENV_E_STATE, "policy HEAD_NETWORK but no head policy network bound (ranenv_set_head_policy_network)");
    if (head_inter(h)) {
        if (!obs_inter) return fail(h, RANENV_E_INVALID, "the policy network reads obs_inter: the step needs that buffer");
        if (!aligned8(obs_inter)) return fail(h, RANENV_E_INVALID, "the replay ring copies dev_obs_inter as 8-byte words: it must be 8-byte aligned");
    } else {
        if (!h->kp.head_obs) return fail(h, RANENV_E_STATE, "the replay ring records dev_obs_head: none is bound (ranenv_bind_head_outputs)");
        if (!aligned8(h->kp.head_obs)) return fail(h, RANENV_E_INVALID, "the replay ring copies dev_obs_head as 8-byte words: it must be 8-byte aligned");
    }
    const Recording rec{nullptr, &h->ring, h->ring.done, h->ring.reward_head, head_reward_cols(h), h->ring_written, h->ring.capacity};
    return rollout_run(h, n_steps, obs_inter, obs_intra, reward, done, stream, &rec);
}

int ranenv_replay_sample(ranenv_handle h, int64_t n, uint64_t seed, uint64_t draw, int32_t reward_col, float *dev_obs, float *dev_action,
                         float *dev_reward, float *dev_next_obs, uint8_t *dev_done, int64_t *dev_index, void *stream)
{
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    if (n < 1 || n > (int64_t)0x7FFFFFFF * (256 / GRP)) return fail(h, RANENV_E_INVALID, "n must be >= 1 (and fit one launch)");
    if (const int rc = head_reward_col_check(h, reward_col); rc != RANENV_OK) return rc;
    if (!dev_obs || !dev_action || !dev_reward || !dev_next_obs || !dev_done) return fail(h, RANENV_E_INVALID, "replay sample: only dev_index may be NULL");
    if (!aligned8(dev_obs) || !aligned8(dev_next_obs)) return fail(h, RANENV_E_INVALID, "replay sample: dev_obs / dev_next_obs must be 8-byte aligned");
    if (!h->ring_on || h->ring_written == 0) return fail(h, RANENV_E_STATE, "the replay ring holds no transitions (ranenv_bind_replay, ranenv_collect_replay)");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    ReplaySampleArgs a{};
    const long long filled = h->ring_written < h->ring.capacity ? h->ring_written : h->ring.capacity;
    a.n = n; a.n_rows = filled * h->cfg.batch; a.B = h->cfg.batch; a.S = h->cfg.n_slices; a.reward_col = reward_col; a.reward_cols = head_reward_cols(h);
    a.seed = seed; a.draw = draw;
    a.ring_obs = h->ring.obs; a.ring_next_obs = h->ring.next_obs; a.ring_action = h->ring.action; a.ring_reward = h->ring.reward_head;
    a.ring_done = h->ring.done;
    a.obs = dev_obs; a.action = dev_action; a.reward = dev_reward; a.next_obs = dev_next_obs; a.done = dev_done; a.index = (long long *)dev_index;
    launch_replay_sample((hipStream_t)stream, a);
    HIP_TRY(h, hipGetLastError());
    return RANENV_OK;
}

int ranenv_set_sac_critics(ranenv_handle h, const ranenv_mlp *q1, const ranenv_mlp *q2, void *stream)
{
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    if (!q1 || !q2) return fail(h, RANENV_E_INVALID, "both SAC critics are required");
    if (q1->n_hidden != q2->n_hidden || q1->activation != q2->activation) return fail(h, RANENV_E_INVALID, "the two SAC critics differ in shape");
    NetBind b[2] = {{&h->sac_q1, &q1, 1, NET_SAC_Q}, {&h->sac_q2, &q2, 1, NET_SAC_Q}};
    if (const int rc = net_plan(h, b, 2); rc != RANENV_OK) return rc;
    for (int l = 0; l <= q1->n_hidden + 1; l++)      // (each critic is valid by itself here)
        if (q1->dims[l] != q2->dims[l]) return fail(h, RANENV_E_INVALID, "the two SAC critics differ in shape (width %d: %d and %d)", l, q1->dims[l], q2->dims[l]);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    return net_commit(h, b, 2, (hipStream_t)stream);
}

int ranenv_sac_targets(ranenv_handle h, int64_t n, const float *dev_next_obs, const float *dev_reward, const uint8_t *dev_done, double gamma,
                       double ent_coef, int32_t stochastic, uint64_t seed, uint64_t draw, float *dev_target, float *dev_next_action,
                       float *dev_next_logp, float *dev_q, void *stream)
{
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    if (n < 1 || n > (int64_t)0x7FFFFFFF * NET_ROWS) return fail(h, RANENV_E_INVALID, "n must be >= 1 (and fit one launch)");
    if (!dev_next_obs || !dev_reward || !dev_done || !dev_target) return fail(h, RANENV_E_INVALID, "SAC targets: next_obs, reward, done and target are required");
    if (!h->head.on || h->head_dist != RANENV_HEAD_DIST_GAUSS_TANH)
        return fail(h, RANENV_E_STATE, "SAC targets need a GAUSS_TANH head actor (ranenv_set_head_policy_network)");
    if (!h->sac_q2.on) return fail(h, RANENV_E_STATE, "no SAC critics bound (ranenv_set_sac_critics)");
    if (h->head.net.prec != RANENV_NET_F32) return fail(h, RANENV_E_STATE, "SAC targets need an f32 head actor: the bound one is a RANENV_NET_BF16 net");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    SacArgs a{};
    a.n = n; a.S = h->cfg.n_slices;
    a.next_obs = dev_next_obs; a.reward = dev_reward; a.done = dev_done;
    a.gamma = gamma; a.ent_coef = ent_coef; a.stochastic = stochastic != 0; a.seed = seed; a.draw = draw;
    a.target = dev_target; a.next_action = dev_next_action; a.next_logp = dev_next_logp; a.q = dev_q;
    const hipError_t le = launch_sac_targets((hipStream_t)stream, h->head.net, h->sac_q1.net, h->sac_q2.net, a);
    if (le != hipSuccess) return fail(h, RANENV_E_HIP, "SAC target launch: %s", hipGetErrorString(le));
    return RANENV_OK;
}

// ---- the SAC update (include/ranenv.h "SAC update"; ranenv_sac.hip) ------------------------------------------------------------------
// What ranenv_sac_bind refuses.  No device call.
static int sac_roles(ranenv_handle h, size_t &lds)
{
    if (!h->head.on || h->head_dist != RANENV_HEAD_DIST_GAUSS_TANH)
        return fail(h, RANENV_E_STATE, "the SAC update needs a GAUSS_TANH head actor (ranenv_set_head_policy_network)");
    if (!h->sac_q1.on || !h->sac_q2.on) return fail(h, RANENV_E_STATE, "the SAC update needs bound critics (ranenv_set_sac_critics)");
    if (h->head.net.prec != RANENV_NET_F32) return fail(h, RANENV_E_STATE, "the SAC update trains float32 nets: the head actor is bf16");
    lds = sac_lds_bytes(h->head.net, h->sac_q1.net);
    if (lds > (size_t)PPO_LDS_MAX)
        return fail(h, RANENV_E_STATE, "the SAC nets need %zu bytes of LDS for the larger net's 32-row activations of all layers, the update has %d", lds, (int)PPO_LDS_MAX);
    return RANENV_OK;
}

// ... and the bound state behind it, or RANENV_E_STATE
static int sac_bound(ranenv_handle h, size_t &lds)
{
    if (!h->sac_on) return fail(h, RANENV_E_STATE, "no SAC state bound, or a binding call of another packed size has ended it (ranenv_sac_bind)");
    return sac_roles(h, lds);
}

// Tensor x (0 actor, 1 q1, 2 q2) of the binding: the weights the update trains, Adam's m and v
static float *sac_w(ranenv_handle h, int x) { return x == 0 ? h->head.w : h->d_sac_q + (size_t)(x - 1) * (size_t)h->sac_q_cap; }
static float *sac_m(ranenv_handle h, int x) { return x == 0 ? h->d_sac_a_opt : h->d_sac_q + (size_t)(1 + x) * (size_t)h->sac_q_cap; }
static float *sac_v(ranenv_handle h, int x) { return x == 0 ? h->d_sac_a_opt + h->sac_a_cap : h->d_sac_q + (size_t)(3 + x) * (size_t)h->sac_q_cap; }

// The live critic x (1, 2) becomes a copy of its bound target; tensor x's moments and counter start again.  On the caller's stream.
static int sac_restart(ranenv_handle h, int x, hipStream_t s)
{
    const size_t f = (size_t)(x == 0 ? h->sac_af : h->sac_qf);
    if (x > 0) HIP_TRY(h, hipMemcpyAsync(sac_w(h, x), (x == 1 ? h->sac_q1 : h->sac_q2).w, sizeof(float) * f, hipMemcpyDeviceToDevice, s));
    HIP_TRY(h, hipMemsetAsync(sac_m(h, x), 0, sizeof(float) * f, s));
    HIP_TRY(h, hipMemsetAsync(sac_v(h, x), 0, sizeof(float) * f, s));
    HIP_TRY(h, hipMemsetAsync(h->d_sac_t + x, 0, sizeof(int32_t), s));
    h->sac_t[x] = 0;
    return RANENV_OK;
}

// A binding call has replaced the head actor or a target critic: a copy of another packed size ends the SAC binding; else that
// tensor starts again (sac_restart: a critic's live copy follows its new target).
static int sac_rebound(ranenv_handle h, ranenv::NetSlot *slot, hipStream_t s)
{
    if (!h->sac_on) return RANENV_OK;
    const int x = slot == &h->head ? 0 : (slot == &h->sac_q1 ? 1 : 2);
    if (net_floats(slot->net) != (x == 0 ? h->sac_af : h->sac_qf)) { h->sac_on = false; return RANENV_OK; }
    return sac_restart(h, x, s);
}

int ranenv_sac_bind(ranenv_handle h, double ent_coef_init, int32_t auto_flag, double target_entropy, int32_t slabs, void *stream)
{
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    size_t lds = 0;
    if (const int rc = sac_roles(h, lds); rc != RANENV_OK) return rc;
    if (slabs < 1 || slabs > 256) return fail(h, RANENV_E_INVALID, "slabs %d (1..256)", slabs);
    if (!(ent_coef_init > 0.0) || !std::isfinite(ent_coef_init)) return fail(h, RANENV_E_INVALID, "the entropy coefficient must be positive and finite");
    if (!std::isfinite(target_entropy)) return fail(h, RANENV_E_INVALID, "the target entropy must be finite");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    const long long af = net_floats(h->head.net), qf = net_floats(h->sac_q1.net), stride = af + 2 * qf;
    if (!h->d_sac_t) {
        if (const int rc = dev_alloc(h, &h->d_sac_t, (size_t)4); rc != RANENV_OK) return rc;
        if (const int rc = dev_alloc(h, &h->d_sac_ent, (size_t)4); rc != RANENV_OK) return rc;
        if (const int rc = dev_alloc(h, &h->d_sac_partial, (size_t)256 * 8); rc != RANENV_OK) return rc;
    }
    if (h->sac_q_cap < qf) {             // (an outgrown one stays allocated, like the weights')
        if (const int rc = dev_alloc(h, &h->d_sac_q, 6 * (size_t)qf); rc != RANENV_OK) return rc;
        h->sac_q_cap = qf;
    }
    if (h->sac_a_cap < af) {
        if (const int rc = dev_alloc(h, &h->d_sac_a_opt, 2 * (size_t)af); rc != RANENV_OK) return rc;
        h->sac_a_cap = af;
    }
    if (h->sac_slab_cap < stride * slabs) {
        if (const int rc = dev_alloc(h, &h->d_sac_slab, (size_t)stride * (size_t)slabs); rc != RANENV_OK) return rc;
        h->sac_slab_cap = stride * slabs;
    }
    HIP_TRY(h, hipMemsetAsync(h->d_sac_slab, 0, sizeof(float) * (size_t)h->sac_slab_cap, s));
    HIP_TRY(h, hipMemsetAsync(h->d_sac_partial, 0, sizeof(double) * 256 * 8, s));
    h->sac_af = af; h->sac_qf = qf; h->sac_slabs = slabs; h->sac_auto = auto_flag != 0; h->sac_target_entropy = target_entropy;
    for (int x = 0; x < 3; x++)
        if (const int rc = sac_restart(h, x, s); rc != RANENV_OK) return rc;
    const float ent[4] = {(float)std::log(ent_coef_init), 0.0f, 0.0f, 0.0f};
    HIP_TRY(h, hipMemcpyAsync(h->d_sac_ent, ent, sizeof(ent), hipMemcpyHostToDevice, s));      // (pageable: staged before the call returns)
    HIP_TRY(h, hipMemsetAsync(h->d_sac_t + 3, 0, sizeof(int32_t), s));
    h->sac_t[3] = 0;
    h->sac_on = true;
    return RANENV_OK;
}

int ranenv_sac_update(ranenv_handle h, int32_t n_steps, int32_t minibatch, int64_t first_row, const float *dev_obs, const float *dev_action,
                      const float *dev_reward, const float *dev_next_obs, const uint8_t *dev_done, double lr, double gamma, double tau, uint64_t seed,
                      uint64_t draw, double *dev_stats, float *dev_grad, float *dev_target, void *stream)
{
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    size_t lds = 0;
    if (const int rc = sac_bound(h, lds); rc != RANENV_OK) return rc;
    if (n_steps < 1 || minibatch < 1) return fail(h, RANENV_E_INVALID, "n_steps %d and minibatch %d must be >= 1", n_steps, minibatch);
    if (first_row < 0) return fail(h, RANENV_E_INVALID, "first_row must be >= 0");
    if (!dev_obs || !dev_action || !dev_reward || !dev_next_obs || !dev_done || !dev_stats)
        return fail(h, RANENV_E_INVALID, "the SAC update needs obs, action, reward, next_obs, done and dev_stats");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t s = (hipStream_t)stream;
    const int S = h->cfg.n_slices;
    const long long af = h->sac_af, qf = h->sac_qf, n = minibatch;
    const int tiles = (int)((n + NET_ROWS - 1) / NET_ROWS), grid = tiles < h->sac_slabs ? tiles : h->sac_slabs;
    SacPassArgs p{};
    p.actor = SacNet{h->head.net, h->head.w};
    p.q[0] = SacNet{h->sac_q1.net, sac_w(h, 1)}; p.q[1] = SacNet{h->sac_q2.net, sac_w(h, 2)};
    p.qt[0] = SacNet{h->sac_q1.net, h->sac_q1.w}; p.qt[1] = SacNet{h->sac_q2.net, h->sac_q2.w};
    p.actor.net.w = p.q[0].net.w = p.q[1].net.w = p.qt[0].net.w = p.qt[1].net.w = nullptr;
    p.slab = h->d_sac_slab; p.slab_stride = af + 2 * qf; p.off[0] = 0; p.off[1] = af; p.off[2] = af + qf;
    p.partial = h->d_sac_partial; p.n = n; p.S = S;
    p.gamma = gamma; p.target_entropy = h->sac_target_entropy; p.seed = seed; p.draw = draw; p.log_ent_coef = h->d_sac_ent;
    for (int g = 0; g < n_steps; g++) {
        const size_t r0 = (size_t)g * (size_t)n;
        const bool last = g == n_steps - 1;
        p.first_row = first_row + (long long)r0;
        p.obs = dev_obs + r0 * (size_t)(10 * S); p.action = dev_action + r0 * (size_t)S; p.reward = dev_reward + r0;
        p.next_obs = dev_next_obs + r0 * (size_t)(10 * S); p.done = dev_done + r0; p.target = dev_target ? dev_target + r0 : nullptr;
        float *grad = last ? dev_grad : nullptr;
        HIP_TRY(h, launch_sac_pass(s, 0, grid, lds, p));
        SacApplyArgs a{};
        a.slab = p.slab; a.slab_stride = p.slab_stride; a.used = grid; a.lr = lr; a.tau = tau; a.n = n;
        a.n_seg = 2;
        for (int x = 1; x <= 2; x++)
            a.seg[x - 1] = SacApplySeg{sac_w(h, x), sac_m(h, x), sac_v(h, x), nullptr, grad ? grad + p.off[x] : nullptr, p.off[x], qf, h->sac_t[x] + 1, SAC_OP_ADAM};
        HIP_TRY(h, launch_sac_apply(s, a));
        HIP_TRY(h, launch_sac_pass(s, 1, grid, lds, p));
        a.n_seg = 3;
        a.seg[0] = SacApplySeg{sac_w(h, 0), sac_m(h, 0), sac_v(h, 0), nullptr, grad, 0, af, h->sac_t[0] + 1, SAC_OP_ADAM};
        a.seg[1] = SacApplySeg{sac_w(h, 1), nullptr, nullptr, h->sac_q1.w, nullptr, 0, qf, 0, SAC_OP_POLYAK};
        a.seg[2] = SacApplySeg{sac_w(h, 2), nullptr, nullptr, h->sac_q2.w, nullptr, 0, qf, 0, SAC_OP_POLYAK};
        a.last = 1; a.auto_coef = h->sac_auto; a.t_ent = h->sac_t[3] + 1;
        a.ent = h->d_sac_ent; a.partial = h->d_sac_partial; a.stats = dev_stats + (size_t)g * 8; a.grad_ent = grad ? grad + af + 2 * qf : nullptr;
        a.dev_t = h->d_sac_t;
        for (int x = 0; x < 4; x++) a.t_new[x] = h->sac_t[x] + (x < 3 || h->sac_auto ? 1 : 0);
        HIP_TRY(h, launch_sac_apply(s, a));
        for (int x = 0; x < 4; x++) h->sac_t[x] = a.t_new[x];
    }
    return RANENV_OK;
}

int ranenv_sac_layout(ranenv_handle h, int64_t *actor_floats, int64_t *critic_floats, int64_t *lds_bytes)
{
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    size_t lds = 0;
    if (const int rc = sac_roles(h, lds); rc != RANENV_OK) return rc;
    if (actor_floats) *actor_floats = net_floats(h->head.net);
    if (critic_floats) *critic_floats = net_floats(h->sac_q1.net);
    if (lds_bytes) *lds_bytes = (int64_t)lds;
    return RANENV_OK;
}

int ranenv_sac_lds_bytes(const ranenv_mlp *actor, const ranenv_mlp *critic, int64_t *bytes)
{
    if (!actor || !critic || !bytes) return fail(nullptr, RANENV_E_INVALID, "null argument");
    PolicyNet net[2] = {};
    if (const int rc = ppo_shape_pair(actor, critic, net); rc != RANENV_OK) return rc;
    *bytes = (int64_t)sac_lds_bytes(net[0], net[1]);
    return RANENV_OK;
}

int ranenv_sac_state(ranenv_handle h, int32_t which, float **dev_m, float **dev_v, int32_t **dev_t, int64_t *floats)
{
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    if (which < 0 || which > 3) return fail(h, RANENV_E_INVALID, "which %d (0 actor, 1 q1, 2 q2, 3 log_ent_coef)", which);
    size_t lds = 0;
    if (const int rc = sac_bound(h, lds); rc != RANENV_OK) return rc;
    if (dev_m) *dev_m = which == 3 ? h->d_sac_ent + 1 : sac_m(h, which);
    if (dev_v) *dev_v = which == 3 ? h->d_sac_ent + 2 : sac_v(h, which);
    if (dev_t) *dev_t = h->d_sac_t + which;
    if (floats) *floats = which == 3 ? 1 : (which == 0 ? h->sac_af : h->sac_qf);
    return RANENV_OK;
}

int ranenv_get_sac_net_weights(ranenv_handle h, int32_t which, ranenv_mlp *out, void *stream)
{
    if (!h || !out) return fail(h, RANENV_E_INVALID, "null argument");
    if (which < 0 || which > 4) return fail(h, RANENV_E_INVALID, "which %d (0 actor, 1 q1, 2 q2, 3 q1_target, 4 q2_target)", which);
    const ranenv::NetSlot *slot = which == 0 ? &h->head : (which == 1 || which == 3 ? &h->sac_q1 : &h->sac_q2);
    const char *who = which == 0 ? "head" : "SAC critic";
    if (!slot->on) return fail(h, RANENV_E_STATE, "no %s net bound", who);
    const float *live = nullptr;
    if (which == 1 || which == 2) {          // (the live critics exist under a binding alone)
        size_t lds = 0;
        if (const int rc = sac_bound(h, lds); rc != RANENV_OK) return rc;
        live = sac_w(h, which);
    }
    return net_export(h, slot, 0, who, out, stream, live);
}

int ranenv_get_sac_log_ent_coef(ranenv_handle h, float *dev_out, void *stream)
{
    if (!h || !dev_out) return fail(h, RANENV_E_INVALID, "null argument");
    size_t lds = 0;
    if (const int rc = sac_bound(h, lds); rc != RANENV_OK) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipMemcpyAsync(dev_out, h->d_sac_ent, sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return RANENV_OK;
}

int ranenv_gae(ranenv_handle h, int32_t n_steps, int32_t n_cols, const double *reward, const float *vf, const uint8_t *done, double gamma,
               double lambda, float *adv, float *vtarg, void *stream)
{
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    if (n_steps < 1 || n_cols < 1) return fail(h, RANENV_E_INVALID, "n_steps and n_cols must be >= 1");
    if (!reward || !vf || !done) return fail(h, RANENV_E_INVALID, "GAE reads reward, vf and done");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    launch_gae((hipStream_t)stream, n_steps, h->cfg.batch, n_cols, reward, n_cols, vf, done, gamma, lambda, adv, vtarg);
    HIP_TRY(h, hipGetLastError());
    return RANENV_OK;
}

int ranenv_gae_population(ranenv_handle h, int32_t n_steps, int32_t n_cols, const double *reward, const float *vf, const uint8_t *done, int32_t n,
                          const double *host_gamma, const double *host_lambda, float *adv, float *vtarg, void *stream)
{
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    if (n_steps < 1 || n_cols < 1) return fail(h, RANENV_E_INVALID, "n_steps and n_cols must be >= 1");
    if (!reward || !vf || !done) return fail(h, RANENV_E_INVALID, "GAE reads reward, vf and done");
    if (const int rc = gae_pairs_check(h, n, host_gamma, host_lambda); rc != RANENV_OK) return rc;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    GaePop g{};
    g.pop = h->pop;
    for (int m = 0; m < n; m++) { g.gamma[m] = host_gamma[m]; g.lambda[m] = host_lambda[m]; }
    launch_gae_pop((hipStream_t)stream, n_steps, h->cfg.batch, n_cols, reward, n_cols, vf, done, g, adv, vtarg);
    HIP_TRY(h, hipGetLastError());
    return RANENV_OK;
}

// ---------------------------------------------------------------------------------------------
// Row lists on the device (include/ranenv.h)
// ---------------------------------------------------------------------------------------------
// What both entries refuse before any device call, and the grouping's env ranges: the population's, or {0, B}
static int rows_check(ranenv_handle h, int32_t n_steps, int32_t grouping, PopMap &map)
{
    if (n_steps < 1) return fail(h, RANENV_E_INVALID, "n_steps must be >= 1");
    if (grouping != RANENV_PPO_ROWS_MEMBERS && grouping != RANENV_PPO_ROWS_SLICES)
        return fail(h, RANENV_E_INVALID, "grouping %d is neither RANENV_PPO_ROWS_MEMBERS nor RANENV_PPO_ROWS_SLICES", grouping);
    if (grouping == RANENV_PPO_ROWS_SLICES && h->pop.n > 1)
        return fail(h, RANENV_E_INVALID, "RANENV_PPO_ROWS_SLICES takes one member: the handle has a population of %d", h->pop.n);
    if (h->cfg.n_slices > POP_MAX) return fail(h, RANENV_E_INVALID, "the row lists take at most %d slices", (int)POP_MAX);
    if ((long long)n_steps * h->cfg.batch * h->cfg.n_slices > 2147483647LL)
        return fail(h, RANENV_E_INVALID, "a record of %d x %d x %d cells is beyond the row lists' int32 limit (2^31 - 1)", n_steps, h->cfg.batch, h->cfg.n_slices);
    map = PopMap{};
    if (grouping == RANENV_PPO_ROWS_MEMBERS && h->pop.n > 0) map = h->pop;
    else { map.n = 1; map.first[0] = 0; map.first[1] = h->cfg.batch; }
    return RANENV_OK;
}

// A device array of the row lists grown to `need` elements (with `slack` on top when it has to move); the outgrown one is freed
static int rows_grow(ranenv_handle h, int32_t **arr, long long *cap, long long need, long long slack)
{
    if (need <= *cap) return RANENV_OK;
    void *ptr = nullptr;
    const hipError_t e = hipMalloc(&ptr, sizeof(int32_t) * (size_t)(need + slack));
    if (e != hipSuccess) return fail(h, RANENV_E_NOMEM, "row lists (%.3f GB): %s", (double)(need + slack) * sizeof(int32_t) / 1e9, hipGetErrorString(e));
    if (*arr) (void)hipFree(*arr);      // (waits for the device: nothing enqueued still reads it)
    *arr = (int32_t *)ptr; *cap = need + slack;
    return RANENV_OK;
}

int ranenv_ppo_row_count(ranenv_handle h, int32_t n_steps, const int8_t *dev_mask_inter, int32_t grouping, int32_t *host_first_inter,
                         int32_t *host_first_intra, void *stream_)
{
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    PopMap map;
    if (const int rc = rows_check(h, n_steps, grouping, map); rc != RANENV_OK) return rc;
    if (!host_first_inter || (dev_mask_inter && !host_first_intra)) return fail(h, RANENV_E_INVALID, "null table (host_first_intra may be NULL without a mask only)");
    ranenv::RowLists &r = h->rows;
    r.valid = false;
    const int B = h->cfg.batch, S = h->cfg.n_slices;
    const bool slices = grouping == RANENV_PPO_ROWS_SLICES;
    // the inter kind: arithmetic
    for (int m = 0; m <= map.n; m++) r.first[0][m] = n_steps * map.first[m];
    // the intra kind's geometry: chunks of one unit each, unit-major
    RowsGeom &g = r.geom;
    g = RowsGeom{};
    g.T = n_steps; g.B = B; g.S = S; g.grouping = grouping; g.units = slices ? S : map.n;
    for (int m = 0; m <= map.n; m++) g.first_env[m] = map.first[m];
    long long chunks = 0;
    for (int u = 0; u < g.units; u++) {
        const long long per = slices ? ((long long)n_steps * B + ROWS_CHUNK - 1) / ROWS_CHUNK
                                     : ((long long)(map.first[u + 1] - map.first[u]) * S + ROWS_CHUNK - 1) / ROWS_CHUNK;
        g.chunk_first[u] = (int)chunks; g.chunks_per[u] = (int)per;
        chunks += slices ? per : per * n_steps;
        if (chunks > 2147483647LL) return fail(h, RANENV_E_INVALID, "the record's cells make more than 2^31 - 1 chunks");
    }
    g.chunk_first[g.units] = g.n_chunks = (int)chunks;
    for (int u = 0; u <= POP_MAX; u++) r.first[1][u] = 0;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t stream = (hipStream_t)stream_;
    if (dev_mask_inter) {
        const long long tab = POP_MAX + 1;
        if (const int rc = rows_grow(h, &r.d_chunks, &r.chunks_cap, 2 * chunks + tab, 0); rc != RANENV_OK) return rc;
        int32_t *counts = r.d_chunks, *offsets = r.d_chunks + chunks, *first = r.d_chunks + 2 * chunks;
        launch_rows_count(stream, g, dev_mask_inter, counts, offsets, first);
        HIP_TRY(h, hipGetLastError());
        HIP_TRY(h, hipMemcpyAsync(r.first[1], first, sizeof(int32_t) * (size_t)(g.units + 1), hipMemcpyDeviceToHost, stream));
        HIP_TRY(h, hipStreamSynchronize(stream));      // the one wait: the caller sizes its lists by these counts
        const long long total = r.first[1][g.units], cells = (long long)n_steps * B * S;
        if (total < 0 || total > cells) return fail(h, RANENV_E_HIP, "row count: %lld live cells of %lld", total, cells);
        if (const int rc = rows_grow(h, &r.d_base, &r.base_cap, std::max(total, 1LL), std::min(cells - total, total / 4 + 1024)); rc != RANENV_OK) return rc;
        launch_rows_compact(stream, g, dev_mask_inter, offsets, r.d_base, total);
        HIP_TRY(h, hipGetLastError());
        for (int u = 0; u <= g.units; u++) host_first_intra[u] = r.first[1][u];
    }
    for (int m = 0; m <= map.n; m++) host_first_inter[m] = r.first[0][m];
    r.valid = true; r.n_steps = n_steps; r.grouping = grouping; r.mask = dev_mask_inter; r.pop = map;
    return RANENV_OK;
}

int ranenv_ppo_row_order(ranenv_handle h, int32_t n_steps, const int8_t *dev_mask_inter, int32_t grouping, int32_t epochs, uint64_t seed,
                         int32_t *dev_order_inter, int32_t *dev_order_intra, void *stream_)
{
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    PopMap map;
    if (const int rc = rows_check(h, n_steps, grouping, map); rc != RANENV_OK) return rc;
    if (epochs < 1) return fail(h, RANENV_E_INVALID, "epochs must be >= 1");
    const ranenv::RowLists &r = h->rows;
    if (!r.valid || r.n_steps != n_steps || r.mask != dev_mask_inter || r.grouping != grouping || memcmp(&map, &r.pop, sizeof(map)) != 0)
        return fail(h, RANENV_E_STATE, "ranenv_ppo_row_order follows a ranenv_ppo_row_count of the same n_steps, mask and grouping under the same population");
    if (dev_order_intra && !dev_mask_inter) return fail(h, RANENV_E_STATE, "the count had no mask: it gave the inter kind alone");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t stream = (hipStream_t)stream_;
    for (int kind = 0; kind < 2; kind++) {
        int32_t *out = kind ? dev_order_intra : dev_order_inter;
        RowsShuffle a{};
        a.kind = kind; a.units = kind ? r.geom.units : map.n; a.B = h->cfg.batch; a.seed = seed;
        a.n = r.first[kind][a.units];
        if (!out || a.n == 0) continue;
        for (int u = 0; u <= a.units; u++) a.first[u] = r.first[kind][u];
        for (int m = 0; m <= map.n; m++) a.first_env[m] = map.first[m];
        a.base = kind ? r.d_base : nullptr; a.out = out;
        launch_rows_shuffle(stream, epochs, a);
        HIP_TRY(h, hipGetLastError());
    }
    return RANENV_OK;
}

// Episode sums of the two head rewards: they exist once episode metrics are enabled AND head rewards are bound; whichever call
// completes the pair allocates (zeroed).
static int head_sums_alloc(ranenv_handle h)
{
    if (!h->kp.acc || !h->kp.head_reward || h->d_head_acc) return RANENV_OK;
    const size_t B = (size_t)h->cfg.batch;
    if (h->ep_slots > 0 && dev_alloc(h, &h->d_head_ep_acc, B * (size_t)h->ep_slots * 2) != RANENV_OK) return RANENV_E_NOMEM;
    return dev_alloc(h, &h->d_head_acc, B * 2);
}

// Per-slice sums, their log and the log's scenario rows (-1: no episode logged in that slot) start from zero
static int slice_sums_zero(ranenv_handle h, hipStream_t stream)
{
    const size_t B = (size_t)h->cfg.batch, n = (size_t)h->cfg.n_slices * RANENV_SLICE_METRIC_COLS;
    HIP_TRY(h, hipMemsetAsync(h->d_slice_acc, 0, sizeof(double) * B * n, stream));
    if (h->d_slice_ep_acc) HIP_TRY(h, hipMemsetAsync(h->d_slice_ep_acc, 0, sizeof(double) * B * (size_t)h->ep_slots * n, stream));
    if (h->d_slice_ep_scn) HIP_TRY(h, hipMemsetAsync(h->d_slice_ep_scn, 0xff, sizeof(int32_t) * B * (size_t)h->ep_slots, stream));
    return RANENV_OK;
}

int ranenv_enable_metrics(ranenv_handle h, int32_t episode_slots, void *stream_)
{
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    if (episode_slots < 0) { h->kp.acc = nullptr; h->slice_on = false; return RANENV_OK; }      // off, the per-slice sums too (what was accumulated stays readable)
    if (h->d_acc && episode_slots != h->ep_slots)
        return fail(h, RANENV_E_STATE, "episode metrics were enabled with %d slots per env", h->ep_slots);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t stream = (hipStream_t)stream_;
    const size_t B = (size_t)h->cfg.batch;
    if (!h->d_acc) {
        if (dev_alloc(h, &h->d_acc, B * 8) != RANENV_OK || dev_alloc(h, &h->d_ep_n, B) != RANENV_OK) return RANENV_E_NOMEM;
        if (episode_slots > 0 && dev_alloc(h, &h->d_ep_acc, B * (size_t)episode_slots * 8) != RANENV_OK) return RANENV_E_NOMEM;
        h->ep_slots = episode_slots;
    }
    HIP_TRY(h, hipMemsetAsync(h->d_acc, 0, sizeof(double) * B * 8, stream));
    HIP_TRY(h, hipMemsetAsync(h->d_ep_n, 0, sizeof(int32_t) * B, stream));
    if (h->d_ep_acc) HIP_TRY(h, hipMemsetAsync(h->d_ep_acc, 0, sizeof(double) * B * (size_t)h->ep_slots * 8, stream));
    h->kp.acc = h->d_acc;
    if (head_sums_alloc(h) != RANENV_OK) return RANENV_E_NOMEM;
    if (h->d_head_acc) HIP_TRY(h, hipMemsetAsync(h->d_head_acc, 0, sizeof(double) * B * 2, stream));
    if (h->d_head_ep_acc) HIP_TRY(h, hipMemsetAsync(h->d_head_ep_acc, 0, sizeof(double) * B * (size_t)h->ep_slots * 2, stream));
    if (h->slice_on) return slice_sums_zero(h, stream);
    return RANENV_OK;
}

static_assert(sizeof(ranenv_trace) == RANENV_TRACE_BYTES, "ranenv_trace: two int32 and 19 pointers");

int ranenv_bind_trace(ranenv_handle h, const ranenv_trace *tr, void *stream_)
{
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    if (!tr) { h->trace_on = false; h->trace = ranenv_trace{}; h->trace_env.clear(); h->trace_slot.clear(); return RANENV_OK; }
    const int B = h->cfg.batch, n = tr->n_envs;
    if (n < 1 || n > B) return fail(h, RANENV_E_INVALID, "trace: n_envs %d outside [1,%d]", n, B);
    if (tr->capacity < 1) return fail(h, RANENV_E_INVALID, "trace: capacity %d < 1", tr->capacity);
    if (!tr->envs) return fail(h, RANENV_E_INVALID, "trace: null env list");
    if ((tr->pkt_incoming || tr->pkt_throughputs) && (h->cfg.flags & RANENV_F_NO_RAW_OUTPUT))
        return fail(h, RANENV_E_INVALID, "trace: pkt_incoming and pkt_throughputs are not available with RANENV_F_NO_RAW_OUTPUT");
    std::vector<std::pair<int32_t, int32_t>> order((size_t)n);
    for (int i = 0; i < n; i++) {
        if (tr->envs[i] < 0 || tr->envs[i] >= B) return fail(h, RANENV_E_INVALID, "trace: env %d (entry %d) outside the batch of %d", tr->envs[i], i, B);
        order[(size_t)i] = {tr->envs[i], i};
    }
    std::sort(order.begin(), order.end());
    for (int i = 1; i < n; i++)
        if (order[(size_t)i].first == order[(size_t)i - 1].first) return fail(h, RANENV_E_INVALID, "trace: env %d is listed twice", order[(size_t)i].first);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t stream = (hipStream_t)stream_;
    int32_t *d = h->d_trace; int cap = h->trace_cap;
    if (n > cap) {
        if (dev_alloc(h, &d, 4 * (size_t)n) != RANENV_OK) return RANENV_E_NOMEM;
        cap = n;
    }
    std::vector<int32_t> words(2 * (size_t)cap, 0);
    for (int i = 0; i < n; i++) { words[(size_t)i] = order[(size_t)i].first; words[(size_t)cap + i] = order[(size_t)i].second; }
    HIP_TRY(h, hipMemcpyAsync(d, words.data(), sizeof(int32_t) * words.size(), hipMemcpyHostToDevice, stream));
    HIP_TRY(h, hipMemsetAsync(d + 2 * (size_t)cap, 0, sizeof(int32_t) * 2 * (size_t)cap, stream));
    HIP_TRY(h, hipStreamSynchronize(stream));
    h->d_trace = d; h->trace_cap = cap;
    h->trace_env.resize((size_t)n); h->trace_slot.resize((size_t)n);
    for (int i = 0; i < n; i++) { h->trace_env[(size_t)i] = order[(size_t)i].first; h->trace_slot[(size_t)i] = order[(size_t)i].second; }
    h->trace = *tr; h->trace.envs = nullptr;       // (the caller's host array is not kept)
    h->trace_on = true;
    return RANENV_OK;
}

int ranenv_get_trace_counts(ranenv_handle h, int32_t **dev_count, int32_t **dev_lost)
{
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    if (!h->trace_on) return fail(h, RANENV_E_STATE, "no trace is bound (ranenv_bind_trace)");
    if (dev_count) *dev_count = h->d_trace + 2 * (size_t)h->trace_cap;
    if (dev_lost) *dev_lost = h->d_trace + 3 * (size_t)h->trace_cap;
    return RANENV_OK;
}

int ranenv_reset_trace(ranenv_handle h, void *stream)
{
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    if (!h->trace_on) return fail(h, RANENV_E_STATE, "no trace is bound (ranenv_bind_trace)");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipMemsetAsync(h->d_trace + 2 * (size_t)h->trace_cap, 0, sizeof(int32_t) * 2 * (size_t)h->trace_cap, (hipStream_t)stream));
    return RANENV_OK;
}

int ranenv_enable_slice_metrics(ranenv_handle h, int32_t enable, void *stream_)
{
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    if (!enable) { h->slice_on = false; return RANENV_OK; }      // off (what was accumulated stays readable)
    if (h->cfg.flags & RANENV_F_NO_RAW_OUTPUT)
        return fail(h, RANENV_E_INVALID, "per-slice metrics read pkt_incoming and pkt_throughputs: not available with RANENV_F_NO_RAW_OUTPUT");
    if (!h->kp.acc) return fail(h, RANENV_E_STATE, "per-slice metrics take their episode slots from ranenv_enable_metrics: call it first");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    const size_t B = (size_t)h->cfg.batch, n = (size_t)h->cfg.n_slices * RANENV_SLICE_METRIC_COLS;
    if (!h->d_slice_acc) {
        if (h->ep_slots > 0 && (dev_alloc(h, &h->d_slice_ep_acc, B * (size_t)h->ep_slots * n) != RANENV_OK ||
                                dev_alloc(h, &h->d_slice_ep_scn, B * (size_t)h->ep_slots) != RANENV_OK)) return RANENV_E_NOMEM;
        if (dev_alloc(h, &h->d_slice_acc, B * n) != RANENV_OK) return RANENV_E_NOMEM;
    }
    h->slice_on = true;
    return slice_sums_zero(h, (hipStream_t)stream_);
}

int ranenv_get_slice_metrics(ranenv_handle h, double **dev_running, double **dev_episode_log, int32_t **dev_episode_scenario, int32_t *n_cols)
{
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    if (!h->d_slice_acc) return fail(h, RANENV_E_STATE, "per-slice metrics are not enabled (ranenv_enable_slice_metrics)");
    if (dev_running) *dev_running = h->d_slice_acc;
    if (dev_episode_log) *dev_episode_log = h->d_slice_ep_acc;
    if (dev_episode_scenario) *dev_episode_scenario = h->d_slice_ep_scn;
    if (n_cols) *n_cols = RANENV_SLICE_METRIC_COLS;
    return RANENV_OK;
}

int ranenv_get_head_metrics(ranenv_handle h, double **dev_running, double **dev_episode_log, int32_t *episode_slots)
{
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    if (dev_running) *dev_running = h->d_head_acc;
    if (dev_episode_log) *dev_episode_log = h->d_head_ep_acc;
    if (episode_slots) *episode_slots = h->d_head_acc ? h->ep_slots : 0;
    return RANENV_OK;
}

int ranenv_get_metrics(ranenv_handle h, double **dev_running, double **dev_episode_log, int32_t **dev_episodes_done, int32_t *episode_slots)
{
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    if (!h->d_acc) return fail(h, RANENV_E_STATE, "episode metrics are not enabled (ranenv_enable_metrics)");
    if (dev_running) *dev_running = h->d_acc;
    if (dev_episode_log) *dev_episode_log = h->d_ep_acc;
    if (dev_episodes_done) *dev_episodes_done = h->d_ep_n;
    if (episode_slots) *episode_slots = h->ep_slots;
    return RANENV_OK;
}

int ranenv_set_traffic_generator(ranenv_handle h, int32_t enable, uint64_t seed, int32_t env_id_base, void *stream_)
{
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    if (!enable) { h->kp.trf_gen = 0; return RANENV_OK; }
    if (env_id_base < 0) return fail(h, RANENV_E_INVALID, "env_id_base must be >= 0");
    h->kp.trf_seed = seed; h->kp.env_id_base = env_id_base;
    h->kp.trf_gen = 1;
    const int rc = build_poisson_tables(h, (hipStream_t)stream_);
    if (rc != RANENV_OK) h->kp.trf_gen = 0;
    return rc;
}

int ranenv_get_poisson_tables(ranenv_handle h, uint64_t *host_cdf, uint8_t *host_guide)
{
    if (!h || !host_cdf || !host_guide) return fail(h, RANENV_E_INVALID, "null argument");
    if (!h->kp.trf_gen || !h->d_pois_cdf) return fail(h, RANENV_E_STATE, "the traffic generator is not enabled");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    HIP_TRY(h, hipDeviceSynchronize());
    HIP_TRY(h, hipMemcpy(host_cdf, h->d_pois_cdf, NS_all(h) * 256 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    HIP_TRY(h, hipMemcpy(host_guide, h->d_pois_guide, NS_all(h) * 64, hipMemcpyDeviceToHost));
    return RANENV_OK;
}

int ranenv_set_max_steps(ranenv_handle h, const int32_t *host_max_steps, void *stream_)
{
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    h->sh_valid = false;           // (`done` of a step already enqueued was decided under the old lengths: the shadow restarts at the next full reset)
    if (!host_max_steps) { h->kp.max_steps_env = nullptr; h->host_max_steps.clear(); return RANENV_OK; }
    for (int b = 0; b < h->cfg.batch; b++) if (host_max_steps[b] < 1) return fail(h, RANENV_E_INVALID, "env %d: max_steps must be >= 1", b);
    if (!h->d_max_steps && dev_alloc(h, &h->d_max_steps, (size_t)h->cfg.batch) != RANENV_OK) return RANENV_E_NOMEM;
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(h, hipMemcpyAsync(h->d_max_steps, host_max_steps, sizeof(int32_t) * (size_t)h->cfg.batch, hipMemcpyHostToDevice, stream));
    HIP_TRY(h, hipStreamSynchronize(stream));
    h->kp.max_steps_env = h->d_max_steps;
    h->host_max_steps.assign(host_max_steps, host_max_steps + h->cfg.batch);
    return RANENV_OK;
}

int ranenv_set_episode_table(ranenv_handle h, const ranenv_episode *host_table, int32_t first_episode, int32_t n_episodes, void *stream_)
{
    if (!h || !host_table) return fail(h, RANENV_E_INVALID, "null argument");
    if (n_episodes < 1 || first_episode < 0) return fail(h, RANENV_E_INVALID, "need n_episodes >= 1 and first_episode >= 0");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    for (int i = 0; i < n_episodes; i++) { const int rc = check_episode(h, host_table[i], "episode table entry", i); if (rc != RANENV_OK) return rc; }
    ranenv_episode *d = nullptr;
    if (dev_alloc(h, &d, (size_t)n_episodes) != RANENV_OK) return RANENV_E_NOMEM;      // (an older table stays allocated until destroy)
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(h, hipMemcpyAsync(d, host_table, sizeof(ranenv_episode) * (size_t)n_episodes, hipMemcpyHostToDevice, stream));
    HIP_TRY(h, hipStreamSynchronize(stream));
    h->d_ep_table = d; h->ep_table_first = first_episode; h->ep_table_n = n_episodes; h->idle_check_dirty = true;
    h->ar_on = false;                      // the rule is re-validated against the new table
    return RANENV_OK;
}

int ranenv_set_autoreset(ranenv_handle h, int32_t enable, int32_t initial_episode, int32_t max_episode, int32_t random_episodes,
                         uint64_t seed, const int32_t *host_episode_no, void *stream_)
{
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    if (!enable) { h->ar_on = false; return RANENV_OK; }
    if (!h->d_ep_table) return fail(h, RANENV_E_STATE, "no episode table (ranenv_set_episode_table)");
    if (initial_episode < h->ep_table_first || max_episode <= initial_episode || max_episode > h->ep_table_first + h->ep_table_n)
        return fail(h, RANENV_E_INVALID, "episodes [%d,%d) must be a non-empty range inside the table [%d,%d)", initial_episode, max_episode,
                    h->ep_table_first, h->ep_table_first + h->ep_table_n);
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t stream = (hipStream_t)stream_;
    if (host_episode_no) {
        for (int b = 0; b < h->cfg.batch; b++)
            if (host_episode_no[b] < h->ep_table_first || host_episode_no[b] >= h->ep_table_first + h->ep_table_n)
                return fail(h, RANENV_E_INVALID, "env %d: episode number %d outside the table", b, host_episode_no[b]);
        HIP_TRY(h, hipMemcpyAsync(ST_episode_no(h->kp), host_episode_no, sizeof(int32_t) * (size_t)h->cfg.batch, hipMemcpyHostToDevice, stream));
        HIP_TRY(h, hipMemsetAsync(ST_reset_count(h->kp), 0, sizeof(int32_t) * (size_t)h->cfg.batch, stream));
        HIP_TRY(h, hipStreamSynchronize(stream));
    }
    h->ar_initial = initial_episode; h->ar_max = max_episode; h->ar_random = random_episodes ? 1 : 0; h->ar_seed = seed;
    h->ar_on = true;
    return RANENV_OK;
}

// The checks of ranenv_autoreset / _part (`part`: the partition of ranenv_autoreset_part, checked in its place among the others)
static int autoreset_ready(ranenv_handle h, const uint8_t *dev_done, const int32_t *part)
{
    if (!h || !dev_done) return fail(h, RANENV_E_INVALID, "null argument");
    if (!h->ar_on) return fail(h, RANENV_E_STATE, "auto-reset is not configured (ranenv_set_autoreset)");
    int rc = part ? check_part(h, *part) : RANENV_OK;
    if (rc != RANENV_OK) return rc;
    rc = check_ready(h, nullptr, nullptr, false);
    if (rc != RANENV_OK) return rc;
    if (!h->kp.se_pool && !(h->se_mode == RANENV_SE_GATHER && h->d_se_mean))
        return fail(h, RANENV_E_STATE, "auto-reset needs a bound SE pool (the reset observes the new episode's first tile)");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    return RANENV_OK;
}

// `due` envs of [lo, hi) ended their episode at the TTI enqueued last (shadow_due, -1 = unknown): false = none did, nothing to
// enqueue (the host follows the step counters, see ranenv::sh_steps); true = enqueue the auto-reset, which the shadow follows --
// unless the device decides by flags the host cannot follow: then the shadow ends here
static bool autoreset_due(ranenv_handle h, int lo, int hi, int due)
{
    if (due == 0) return false;
    if (due < 0) h->sh_valid = false;
    else shadow_reset_due(h, lo, hi);
    return true;
}

// Enqueue the advance kernel of envs [e0, e0 + n) on `s`; returns the KP of the reset that has to follow it
static KP autoreset_advance(ranenv_handle h, int e0, int n, const uint8_t *dev_done, float *obs_inter, float *obs_intra,
                            float *term_obs_inter, float *term_obs_intra, float *term_obs_head, hipStream_t s)
{
    AdvanceArgs a = advance_args(h, dev_done, obs_inter, obs_intra, term_obs_inter, term_obs_intra, term_obs_head);
    a.e0 = e0;
    h->pclass_maybe = true;                      // (scenarios of the restarted envs, if any: the advance kernel sets the device's flag)
    launch_advance(s, (unsigned)n, a);
    return reset_behind(h, call_kp(h, obs_inter, obs_intra, nullptr, nullptr));
}

int ranenv_autoreset(ranenv_handle h, const uint8_t *dev_done, float *obs_inter, float *obs_intra,
                     float *term_obs_inter, float *term_obs_intra, float *term_obs_head, void *stream_)
{
    const int rc = autoreset_ready(h, dev_done, nullptr);
    if (rc != RANENV_OK) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    const int B = h->cfg.batch;
    if (!autoreset_due(h, 0, B, shadow_due(h, 0, B, dev_done, stream))) return RANENV_OK;
    const KP kp = autoreset_advance(h, 0, B, dev_done, obs_inter, obs_intra, term_obs_inter, term_obs_intra, term_obs_head, stream);
    const hipError_t e = launch<MODE_RESET>(h, kp, stream);
    if (e != hipSuccess) return fail(h, RANENV_E_HIP, "auto-reset launch: %s", hipGetErrorString(e));
    return RANENV_OK;
}

int ranenv_autoreset_part(ranenv_handle h, int32_t part, const uint8_t *dev_done, float *obs_inter, float *obs_intra,
                          float *term_obs_inter, float *term_obs_intra, float *term_obs_head, void *stream_)
{
    int rc = autoreset_ready(h, dev_done, &part);
    if (rc != RANENV_OK) return rc;
    hipStream_t stream = (hipStream_t)stream_, ps = h->part_stream[(size_t)part];
    const int e0 = h->part_lo[(size_t)part], n = h->part_lo[(size_t)part + 1] - e0;
    if (!autoreset_due(h, e0, e0 + n, stream_capturing(stream) ? -1 : shadow_due(h, e0, e0 + n, dev_done, ps))) {
        HIP_TRY(h, hipEventRecord(h->part_done[(size_t)part], ps));                    // ranenv_wait_part still finds its event
        return RANENV_OK;
    }
    rc = part_handoff(h, part, stream);
    if (rc != RANENV_OK) return rc;
    const KP kp = autoreset_advance(h, e0, n, dev_done, obs_inter, obs_intra, term_obs_inter, term_obs_intra, term_obs_head, ps);
    const hipError_t e = launch_range<MODE_RESET>(h, kp, e0, n, ps);
    if (e != hipSuccess) return fail(h, RANENV_E_HIP, "auto-reset launch (partition %d): %s", part, hipGetErrorString(e));
    HIP_TRY(h, hipEventRecord(h->part_done[(size_t)part], ps));
    return RANENV_OK;
}

int ranenv_get_views(ranenv_handle h, ranenv_views *out)
{
    if (!h || !out) return fail(h, RANENV_E_INVALID, "null argument");
    const KP &k = h->kp;
    h->sh_valid = false;           // (the views are writable, step_number included: the host's shadow of the counters ends here; the next full reset restarts it)
    out->pkt_incoming = ST_pkt_incoming(k); out->pkt_throughputs = ST_pkt_throughputs(k);
    out->pkt_effective_thr = ST_pkt_effective_thr(k); out->dropped_pkts = ST_dropped_pkts(k);
    out->queue_pkts = ST_queue_pkts(k); out->queue_age_sum = ST_queue_age_sum(k);
    out->rb_start = ST_rb_start(k); out->rb_count = ST_rb_count(k); out->se_mean = ST_se_mean(k);
    out->win_sent = ST_win_sent(k); out->win_dropped = ST_win_dropped(k);
    out->step_number = ST_step_no(k); out->hist_len = ST_hist_len(k);
    out->mask_inter = ST_mask_inter(k); out->mask_intra = ST_mask_intra(k); out->policy_scores = ST_policy_scores(k);
    out->episode_number = ST_episode_no(k);
    out->episodes = reinterpret_cast<int32_t *>(h->d_episodes);
    return RANENV_OK;
}

int ranenv_bind_head_outputs(ranenv_handle h, float *dev_obs_head, double *dev_reward_head)
{
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    if ((dev_obs_head || dev_reward_head) && (h->cfg.flags & RANENV_F_NO_RAW_OUTPUT))
        return fail(h, RANENV_E_STATE, "the heads read pkt_throughputs: not available with RANENV_F_NO_RAW_OUTPUT");
    h->kp.head_obs = dev_obs_head; h->kp.head_reward = dev_reward_head;
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    return head_sums_alloc(h);
}

int ranenv_set_slice_usecase(ranenv_handle h, int32_t first, int32_t count, const int32_t *usecase, void *stream_)
{
    if (!h || !usecase) return fail(h, RANENV_E_INVALID, "null argument");
    if (first < 0 || count < 1 || first + count > h->cfg.n_scenarios) return fail(h, RANENV_E_INVALID, "scenario rows [%d,%d) outside pool of %d", first, first + count, h->cfg.n_scenarios);
    const size_t n = (size_t)count * h->cfg.n_slices;
    for (size_t i = 0; i < n; i++) if (usecase[i] < 0 || usecase[i] > 3) return fail(h, RANENV_E_INVALID, "use-case bits must be in [0,3]");
    HIP_TRY(h, hipSetDevice(h->cfg.device));
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(h, hipMemcpyAsync(TB_slice_usecase(h->kp) + (size_t)first * h->cfg.n_slices, usecase, n * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    HIP_TRY(h, hipStreamSynchronize(stream));
    return RANENV_OK;
}

int ranenv_se_from_power(const double *dev_power, float *dev_se, int64_t n_elems, double tx_power_per_rb,
                         double noise_power, void *stream)
{
    if (!dev_power || !dev_se) return fail(nullptr, RANENV_E_INVALID, "null argument");
    if (n_elems < 0) return fail(nullptr, RANENV_E_INVALID, "negative element count");
    if (!(noise_power > 0.0)) return fail(nullptr, RANENV_E_INVALID, "noise_power must be positive");
    if (n_elems == 0) return RANENV_OK;
    long long blocks = (n_elems + 511) / 512;
    if (blocks > 256 * 64) blocks = 256 * 64;          // grid-stride beyond 64 workgroups per CU
    launch_se_from_power((hipStream_t)stream, (unsigned)blocks, dev_power, dev_se, (long long)n_elems, tx_power_per_rb, noise_power);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(nullptr, RANENV_E_HIP, "se_from_power launch: %s", hipGetErrorString(e));
    return RANENV_OK;
}

int ranenv_packed_step_fits(const ranenv_config *cfg, int64_t traffic_rows, int64_t se_tiles)
{
    if (!cfg || traffic_rows < 0 || se_tiles < 0) return fail(nullptr, RANENV_E_INVALID, "null / negative argument");
    return pack_fits_32_of(*cfg, (long long)traffic_rows, (long long)se_tiles) ? 1 : 0;
}

int ranenv_selftest_ddiv(const double *dev_a, const double *dev_b, double *dev_fast, double *dev_ieee, int64_t n, void *stream)
{
    if (!dev_a || !dev_b || !dev_fast || !dev_ieee) return fail(nullptr, RANENV_E_INVALID, "null argument");
    if (n < 0) return fail(nullptr, RANENV_E_INVALID, "negative element count");
    if (n == 0) return RANENV_OK;
    launch_ddiv_selftest((hipStream_t)stream, dev_a, dev_b, dev_fast, dev_ieee, (long long)n);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(nullptr, RANENV_E_HIP, "ddiv self-test launch: %s", hipGetErrorString(e));
    return RANENV_OK;
}

int ranenv_launch_info(ranenv_handle h, int32_t *grid, int32_t *block, int32_t *lds_bytes)
{
    if (!h) return fail(h, RANENV_E_INVALID, "null handle");
    if (grid) *grid = h->cfg.batch;
    if (block) *block = h->nt;
    if (lds_bytes) *lds_bytes = (int32_t)shared_core_bytes(h->np);
    return RANENV_OK;
}

}  // extern "C"

