// ppo-libtorch_amd/csrc/api.hip -- the C-ABI of include/ppo_hip.h: context, buffers, launch sequencing, RCCL.
//
// Host language is C++ because the reference is C++; nothing here depends on LibTorch.  The context owns
// every device buffer (allocated once in ppo_ctx_create) and one HIP stream; every entry point only enqueues work.
#include <dlfcn.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <map>
#include <memory>
#include <mutex>
#include <vector>

#include "generic.hpp"
#include "gauss_fused.hpp"
#include "ppo_internal.hpp"
#include "trunc_events.hpp"

// ---------------------------------------------------------------------------------------------------------
// RCCL, bound lazily (single-GPU use never loads it).  One all-reduce per optimizer step.
// ---------------------------------------------------------------------------------------------------------
namespace rccl {
typedef struct { char internal[128]; } UniqueId;
typedef void* Comm;
typedef int (*GetUniqueId_t)(UniqueId*);
typedef int (*CommInitRank_t)(Comm*, int, UniqueId, int);
typedef int (*AllReduce_t)(const void*, void*, size_t, int, int, Comm, hipStream_t);
typedef int (*CommDestroy_t)(Comm);
typedef const char* (*GetErrorString_t)(int);
static GetUniqueId_t GetUniqueId;
static CommInitRank_t CommInitRank;
static AllReduce_t AllReduce;
static CommDestroy_t CommDestroy;
static GetErrorString_t GetErrorString;
static const int kFloat32 = 7, kFloat64 = 8, kSum = 0;
static bool load(std::string& err) {
    static std::mutex mu;
    std::lock_guard<std::mutex> g(mu);
    if (AllReduce) return true;
    void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);  // reuse the copy a host process (e.g. PyTorch) already mapped
    if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) { err = std::string("cannot load librccl: ") + dlerror(); return false; }
    GetUniqueId = (GetUniqueId_t)dlsym(h, "ncclGetUniqueId");
    CommInitRank = (CommInitRank_t)dlsym(h, "ncclCommInitRank");
    AllReduce = (AllReduce_t)dlsym(h, "ncclAllReduce");
    CommDestroy = (CommDestroy_t)dlsym(h, "ncclCommDestroy");
    GetErrorString = (GetErrorString_t)dlsym(h, "ncclGetErrorString");
    if (!GetUniqueId || !CommInitRank || !AllReduce || !CommDestroy) { err = "librccl lacks nccl* symbols"; AllReduce = nullptr; return false; }
    return true;
}
}  // namespace rccl

// ---------------------------------------------------------------------------------------------------------
// In-process communicator: several contexts of ONE process (one host thread each) on one or more GPUs.  Same semantics as
// the RCCL path -- every rank calls the all-reduce, the sum is formed in rank order (deterministic) -- without any RCCL:
// the last rank to arrive runs one kernel on its own stream that reads every rank's buffer and writes the sum back to all.
// ---------------------------------------------------------------------------------------------------------
struct LocalGroup {
    int n = 0;
    int device = -1;              // every member lives on this device (ppo_comm_init_local rejects others)
    std::mutex mu;
    std::condition_variable cv;
    int arrived = 0, joined = 0;
    uint64_t generation = 0;
    bool failed = false;          // a member's launch failed inside the rendezvous: every waiter returns PPO_ERR_COMM instead of hanging
    void* bufs[8] = {};
    hipEvent_t ready[8] = {};
    hipEvent_t done[2] = { nullptr, nullptr };
    ~LocalGroup() { for (hipEvent_t e : done) if (e) (void)hipEventDestroy(e); }
};
// ---------------------------------------------------------------------------------------------------------
// One-shot direct exchange: the all-reduce of a latency-bound payload (36.6 KB of gradient per optimizer step) WITHOUT a
// ring.  Every rank owns a small exchange buffer in fine-grained device memory -- two slots of payload + a flag each -- that its peers
// map through HIP IPC handles (one process per GPU; over xGMI each peer is one point-to-point hop).  An all-reduce is ONE kernel per rank:
// publish the own payload and flag, then for every rank in rank order wait for its flag and add its payload -- a fixed order, so every rank
// forms bit-identical sums -- straight out of the peer's memory.  Two slots suffice: a rank overwrites slot s two calls later, and it cannot
// get there before every peer has finished reading the call in between (whose sum it needed to proceed).
// RCCL stays available (ppo_comm_init); this path is chosen by ppo_comm_init_exchange.
// ---------------------------------------------------------------------------------------------------------
struct ExchangeComm {
    void* own = nullptr;              // [2 parities][8 source ranks][slot_bytes] payload slots the PEERS write into, then flags and counters
                                      // (fine-grained device memory of this rank; layout: kernels_update.hip, xchg_slot)
    size_t slot_bytes = 0;
    void* peer[8] = {};               // mapped exchange buffers of every rank (peer[rank] == own)
    bool opened[8] = {};
    uint64_t seq = 0;                 // calls so far (same on every rank)
    int32_t* timeout_flag = nullptr;  // device int32[4]: [0] set by a kernel whose bounded wait for a peer ran out; [2..3] = the wait limit as a u64 in
                                      // ticks of the 100 MHz counter (kernels_update.hip: xchg_wait_all)
    double wait_seconds = 30.0;       // larger than any realistic host-side skew between ranks (checkpoint write, statistics read-back, code-object load)
};
struct XchgPtrs { void* p[8]; };
hipError_t launch_exchange_allreduce(void* buf, size_t count, bool f64, const XchgPtrs& peers, int rank, int n, size_t slot_bytes, uint64_t seq,
                                     int32_t* timeout_flag, hipStream_t s);
static std::map<int64_t, std::shared_ptr<LocalGroup>> g_local_groups;
static std::mutex g_local_groups_mu;
struct PtrPack { void* p[8]; };
hipError_t launch_local_allreduce(const PtrPack& pk, int n, size_t count, bool f64, hipStream_t s);

// pinned host block a statistics snapshot lands in (device pieces first, then the host-side training state at snapshot time)
struct StatsSnap {
    StepStats st;
    double cf[2];
    double ev[PPO_EV_BLOCKS * 4];
    EpisodeRing ring;
    double gstats[PPO_GSTAT_DOUBLES];
    int32_t error_flag, xchg_flag;
    int64_t es_applied;   // early stop: the applied optimizer steps as the last update's epilogue left them (copied only while that update is unresolved)
    // host side
    int64_t es_nominal;   // ... and what the host counted for the same steps (0 with es_applied 0: opt_step is exact)
    bool have_step, have_ev, have_gstats;
    int world;
    int64_t B, global_step, opt_step, updates;
    double lr;
};

// One device list of truncation events, (flat index t * N + n, V(final obs)), that a fold kernel appends to with one atomicAdd per workgroup.  A context holds
// three: one for its own env (ppo_env_truncation_bootstrap) and two for device-fed rollouts (ppo_dev_observe with flags), used by alternate rollouts so that
// the last CLOSED rollout's events stay readable while the next one is fed.  A list is made by the first call that needs it and kept (the allocation policy of
// ppo_ctx_create in ppo_hip.h).  Its life, one rollout at a time (events_* below): clear the counter in stream order in front of the rollout's first fold;
// hand count / index / value / cap to every fold launch; close -- copy the counter to the pinned word and record the event, behind the last fold; read --
// wait for THAT event only (the update behind it keeps running), copy the entries, sort them by index on the host (trunc_events.hpp) and keep them.
struct DevEventList {
    int32_t* count = nullptr;     // device [1] (+ padding)
    int32_t* count_h = nullptr;   // pinned [1]
    int32_t* index = nullptr;
    float* value = nullptr;
    int64_t cap = 0;              // entries of index / value; 0 until every piece is there
    hipEvent_t ev = nullptr;      // behind the rollout's last fold and the copy of its counter
    bool closed = false;          // the last rollout folded into this list, and its folds and the counter copy are behind ev
    bool fetched = false;         // ... and its events are in idx / val already (sorted by index)
    std::vector<int32_t> idx;
    std::vector<float> val;
};

struct ppo_ctx {
    ppo_config cfg{};
    NetLayout L{};
    LossParams hp{};
    hipStream_t stream = nullptr;
    // generic networks in bf16 storage: the critic's forward and backward passes of a minibatch step run on a second stream beside the actor's
    hipStream_t stream2 = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_gather = nullptr;
    // ppo_update tells a minibatch step which rows the NEXT step will gather (nullptr: none): the step requests that gather on the second stream once its
    // own backward passes are done, beside its reduction / optimizer tail; gen_pre_* = what has been gathered ahead
    const int32_t* gen_next_idx = nullptr; int64_t gen_next_M = 0;
    const int32_t* gen_pre_idx = nullptr; int64_t gen_pre_M = 0;
    std::string err;
    int T = 0, N = 0, O = 0, H = 0, A = 0;
    int64_t B = 0, MB = 0;
    int n_mb = 0, steps_per_update = 0;
    int world = 1, rank = 0;
    rccl::Comm comm = nullptr;
    std::shared_ptr<LocalGroup> lgroup;   // in-process communicator (exclusive with comm)
    hipEvent_t lg_ready = nullptr;
    std::unique_ptr<ExchangeComm> xchg;   // one-shot direct exchange over IPC peer buffers (exclusive with comm / lgroup)

    std::vector<void*> allocs;
    void* buf[PPO_BUF_COUNT_] = {};
    size_t buf_bytes[PPO_BUF_COUNT_] = {};

    float* reset_table = nullptr;
    int reset_cap = 0;
    int32_t* error_flag = nullptr;
    float* slab = nullptr;
    double* stat_slab = nullptr;
    double* loss_sums = nullptr;
    float4* adv_norm = nullptr;         // [steps_per_update + 1] { mean, 1 / (std + 1e-8), std, 0 } per minibatch slot, from adv_stats once per update
    AdvStat* adv_stats = nullptr;       // [steps_per_update] + 1 scratch slot; sits right BEHIND gstats so that one all-reduce per update carries both
    double* gstats = nullptr;           // [PPO_GSTAT_DOUBLES] job-global statistics block of a sharded run (ppo_internal.hpp: PPO_GSTAT_*)
    bool have_gstats = false;           // the block holds the all-reduced statistics of the last ppo_update
    AdamCoef* adam_coefs = nullptr;     // device [steps_per_update + 1]
    AdamCoef* adam_coefs_h = nullptr;   // pinned mirror, two halves used alternately
    hipEvent_t coef_copied[2] = { nullptr, nullptr };  // H2D copy of each half has completed
    int coef_half = 0;
    StepStats* step_stats = nullptr;    // device [steps_per_update + 1]
    double* clipfrac_accum = nullptr;   // {sum, count}
    double* norm2 = nullptr;            // [12] per-tensor squared gradient norms of the current step
    double* ev_sums = nullptr;          // [PPO_EV_BLOCKS][4]
    float* rec_critic = nullptr;        // [B][16] packed sample records the matrix-core update kernel gathers from (launch_pack_records): critic | actor per sample
    float* rec_actor = nullptr;         // = rec_critic + 8 (not an allocation of its own)
    int32_t* row_counts = nullptr;      // [T]
    uint64_t* group_bits = nullptr;     // [T, ceil(N/64)] ballots of finished episodes
    EpisodeRing* ring = nullptr;
    unsigned int* pair_tickets = nullptr;   // [0] values_ring_mfma_kernel's, [1] pack_perm_stats_kernel's last-arriver tickets: 0 between launches
    bool separate_launches = false;    // PPO_KERNEL_SEPARATE_LAUNCHES
    float* scratch_obs = nullptr;       // [N,O] staging for AoS<->SoA conversions
    // ppo_evaluate's scratch, allocated on first use and kept (grown when a call asks for more episodes): per-episode results and, for CartPole, the
    // evaluation reset table (rows of ppo_cartpole_reset_stream_h(eval_table_seed, .); the host copy is kept so that a larger n extends, not redraws)
    float* eval_ret = nullptr;
    int32_t* eval_len = nullptr;        // [eval_cap] lengths, then [eval_cap] truncated flags
    int64_t eval_cap = 0;
    float* eval_table = nullptr;
    int64_t eval_table_cap = 0, eval_table_rows = 0, eval_table_seed = 0;
    std::vector<float> eval_table_h;
    int max_blocks_per_net = 0;
    bool use_mfma = true;
    bool update_single_wave = false;   // PPO_KERNEL_UPDATE_ONE_WAVE
    bool rollout_vector = false;       // PPO_KERNEL_ROLLOUT_VECTOR
    // fp16 range of the matrix-core kernels (ppo_internal.hpp: weight_range_kernel): maxima of |parameter| by class, taken once per update, on the device and mirrored into pinned
    // host memory that the dispatch reads WITHOUT synchronising; wrange_dirty = the host wrote parameters since they were last computed from scratch
    uint32_t* wr_dev = nullptr;
    uint32_t* wr_host = nullptr;       // hipHostMalloc'ed, mapped: wr_host_dev is the device's address of the same words
    uint32_t* wr_host_dev = nullptr;
    hipStream_t wr_stream = nullptr;   // the once-per-update sweep runs here, beside the update's first launches (sweep_weight_range)
    bool wrange_dirty = true;
    float wr_cache[3] = { 0.0f, 0.0f, 0.0f };   // the mirror as last read: the pinned words are uncached for the host (~0.3 us a read), so they are read once per
    bool gen_opt_fused_ok = false;             // generic bf16 path: the last backward pass left the sums of squares gen_opt_fused needs, and nothing touched the gradient since
    bool gen_obs_bf_valid = false;             // generic bf16 path: GenericCtx::obs_bf holds THIS update's observations (set by the update's first step)
    bool wr_in_update = false;                 // rollout / update / stand-alone step, not per launch (an update moves a weight by less than 40 lr: the thresholds' margin)
    int64_t vector_fallback_launches = 0;   // launches that took a vector kernel because a weight did not fit fp16 (ppo_profile.vector_fallback_launches)
    // PPO_KERNEL_GAUSS_FUSED (kernels_gauss_fused.hip): the Gaussian 2 x 64 context's act / critic / minibatch kernels, their launch counts since creation
    // (ppo_gauss_fused_launches) and the update kernel's partial slabs [2][GAUSS_FUSED_MAX_BLOCKS][gauss_fused_slab_stride]
    bool gauss_fused = false;
    // PPO_KERNEL_CAT_FUSED: the categorical twin on the same kernel family; it shares the counters (ppo_gauss_fused_launches reads them for either flag) and the slabs
    bool cat_fused = false;
    // PPO_KERNEL_ENV_GENERIC: CartPole / MountainCar (their own env kernels, state layout and reset table) under a network in the generic engine's layout
    bool env_generic = false;
    // a device env of the fused families: its row (gauss_fused.hpp: FusedEnvInfo), looked up once by ppo_ctx_create; null on every other env
    const FusedEnvInfo* env = nullptr;
    // PPO_KERNEL_ENV_CUT_STATE (a fused device env only): the cut-off record, f32 [env->state + 1, B] -- the KEEP rollout writes column t N + env where that
    // step's episode reached the limit (the pre-reset state, then 0.0f / 1.0f "the env itself terminated"), and cut_state_fold_kernel reads exactly those
    // columns; never cleared, not a PPO_BUF_*; null on every other context
    float* cut_state = nullptr;
    int64_t gf_launches[3] = { 0, 0, 0 };
    float* gf_slab = nullptr;
    unsigned long long* stamps = nullptr;  // [2][12] phase cycles of the diagnostic kernel variant
    // caller-stepped envs (PPO_ENV_HOST: ppo_host_*).  The staging block is pinned host memory the GPU can read: ppo_host_observe copies the caller's step
    // outputs into it (no launch), the next launch commits them reading the block in place (measured faster than one async copy of it ahead of every
    // launch at N = 256 .. 16384: DESIGN.md section 6a).  Layout (host_stage_layout): [obs N*O f32 | reward N f32 | done N i32 | fin_len N i32 | fin_rew N f32 | mask N*A u8]
    bool host_env = false;
    int host_phase = 0;               // 0: no rollout open, 1: ppo_host_act is next, 2: ppo_host_observe is next
    int host_t = 0;                   // steps acted on in the open rollout
    bool host_staged = false;         // step host_t - 1 is staged and not committed yet
    bool host_fin_given = false;
    bool host_as16 = false;           // rollout16_kernel's arithmetic for the whole open rollout (decided by ppo_host_rollout_begin)
    unsigned char* host_stage = nullptr;       // hipHostMalloc'ed, mapped
    unsigned char* host_stage_dev = nullptr;   // the device's address of the same bytes
    size_t host_stage_bytes = 0;
    int64_t* host_act = nullptr;               // i64 [N,H] actions, pinned and mapped: the act kernel writes them with plain stores
    int64_t* host_act_dev = nullptr;
    // env groups (ppo_host_rollout_begin_groups): host_n_groups > 0 while a grouped rollout is open (host_phase stays 1 then: "a rollout is open").  A group
    // owns rows [row0, row0 + rows) of every per-env array, the staging block and the action block included, and its own place in the rollout.
    struct HostGroup {
        int row0 = 0, rows = 0;
        int t = 0;                    // steps acted on
        int phase = 1;                // 1: ppo_host_group_act is next, 2: ppo_host_group_actions, 3: ppo_host_group_observe
        bool staged = false;          // step t - 1 is staged and not committed yet
        bool fin_given = false;
        hipEvent_t ev = nullptr;      // recorded behind the group's act; ppo_host_group_actions waits for it (created with the context, timing disabled)
    };
    int host_n_groups = 0;
    HostGroup host_grp[PPO_HOST_MAX_GROUPS];
    // truncation events (ppo_host_observe_truncated / ppo_host_group_observe_truncated): the episodes of the open rollout that a time limit cut off, as
    // (flat index t * N + n, final observation).  One pinned host block and one device block of the same layout, [index i32 cap | final obs f32 cap * O |
    // value f32 cap], allocated by the first call that carries an event and grown by doubling up to T * N entries (trunc_reserve).  The observes append to
    // the front of the host block and launch nothing; ppo_host_rollout_end sorts the list, copies it over once and folds gamma * V(final obs) into REWARDS
    // (host_fold_truncations).  The value area of the host block holds the values of the last closed rollout, copied back behind the fold.
    unsigned char* trunc_h = nullptr;
    unsigned char* trunc_dev = nullptr;
    int64_t trunc_cap = 0;
    int64_t trunc_n = 0;                   // events of the open rollout
    std::vector<int32_t> trunc_last_idx;   // the last closed rollout's, ascending (ppo_host_truncations)
    hipEvent_t trunc_ev = nullptr;         // behind the fold and the copy of its values (created with the blocks, timing disabled)
    std::vector<int32_t> trunc_order;      // sorting scratch, kept
    std::vector<float> trunc_sorted;
    // caller-stepped envs on the device (ppo_dev_*): a rollout is host-fed or device-fed as a whole, decided by its first act.  A device-fed step is
    // committed by ppo_dev_observe at once (host_staged stays false), and its truncation events go to one of two lists (DevEventList).
    int host_feed = 0;                // the open rollout: 0 = no act yet, 1 = host-fed (ppo_host_act), 2 = device-fed (ppo_dev_act)
    hipEvent_t dev_ev_in = nullptr, dev_ev_out = nullptr;   // the hand-over between the caller's stream and the context's (created by the first call that needs them)
    DevEventList dev_events[2];
    int dev_list = 0;                 // the list of the open (else: the last) device-fed rollout
    bool dev_list_used = false;       // the open rollout has enqueued a fold (the list's counter was cleared in front of it)
    int dev_last = -1;                // >= 0: the last closed rollout was device-fed and enqueued folds into this list
    // time-limit truncations of the context's own device env (ppo_env_truncation_bootstrap): off unless that call turned it on.  With the switch on,
    // ppo_rollout enqueues the fold behind the value launch and closes the list at once (env_fold_truncations).
    bool envt_on = false;
    DevEventList env_events;
    // observation normalisation (ppo_obs_norm_*): off unless ppo_obs_norm_enable turned it on.  The statistics (f64 mean[O] | var[O]) and the two [N,O]
    // scratches (the normalised step the commit reads; the normalised final observations of a device-fed fold) are allocated by the first call that needs
    // them and kept; the row count lives here, on the host: it grows by the batch's rows per update.
    int on_mode = 0;                  // 0 off, 1 update + apply, 2 apply only
    float on_clip = 10.0f, on_eps = 1e-8f;
    double on_count = 0.0;
    double* on_stats = nullptr;
    float* on_obs = nullptr;
    float* on_final = nullptr;
    // reward normalisation (ppo_reward_norm_*): off unless ppo_reward_norm_enable turned it on.  The accumulators (f64 ret[N]), the statistics (f64
    // mean | var of the discounted returns) and the [N] scratch the commit stores in the reward row are allocated by the first call that needs them and
    // kept; the count of merged returns lives here, on the host.
    int rn_mode = 0;                  // 0 off, 1 update + apply, 2 apply only
    float rn_clip = 10.0f, rn_eps = 1e-8f;
    double rn_count = 0.0;
    double* rn_ret = nullptr;
    double* rn_stats = nullptr;
    float* rn_rew = nullptr;
    // PPO_KERNEL_ENV_REWARD_NORM (a fused device env only): the f64 workspace of the whole-rollout normaliser, rewnorm_rollout_workspace(N, T) doubles --
    // R [T, N], the batch moments [2, T] and the statistics a rollout started from [2]; made by ppo_ctx_create under the flag, no PPO_BUF_*.  Null: the
    // three ppo_reward_norm_* calls refuse a device-env context (rn_state)
    double* rn_ws = nullptr;
    GenericCtx* gen = nullptr;       // non-null: synthetic env / network other than 2 x 64 (generic.hpp); every L-dependent entry point dispatches on it
    uint8_t* cur_mask = nullptr;     // generic path: action mask of the observation in NEXT_OBS, [N, A]
    bool force_collectives = false;  // PPO_COMM_SELFTEST: world == 1 but the multi-rank path (RCCL included) is taken
    double* fused_partial = nullptr; // [fused_opt_blocks][12] per-workgroup sums of squares of the gradient
    int last_n_blocks[2] = { 0, 0 };
    int prof_every = 1;              // mode 2: bracket one update-kernel launch in prof_every (an event pair costs the stream ~3 us)
    int64_t prof_count = 0;
    bool prof_last_sampled = false;   // the last update launch was bracketed: so is the all-reduce that follows it
    bool stamping = false;           // diagnostic flavour of the update kernel (in-kernel phase stamps)

    // host-side training state
    double lr = 0.0;
    int64_t opt_step = 0;
    int64_t global_step = 0;
    int64_t updates = 0;
    int64_t num_updates_total = 0;
    int64_t rollout_steps = 0;      // sampling-stream position (rollout steps taken so far)
    int64_t act_calls = 0;
    bool fin_pending = false;
    bool have_ev = false;
    int last_stat_slot = -1;
    double last_global_M = 1.0;

    // early stop at a target KL (ppo_target_kl_set; kernels_earlystop.hip).  Nothing here is allocated, and nothing is launched, until a positive target is set.
    // An update with a target counts every enqueued step in opt_step (es_nominal = its value behind the loop) and leaves es_pending set; es_resolve
    // waits for that update's epilogue only and takes the steps it did not apply off opt_step and the epochs off epochs_total.
    double target_kl = 0.0;
    EarlyStopDev* es_dev = nullptr;
    EarlyStopHost* es_host = nullptr;   // pinned; the head of *es_dev as the last update with a target left it
    hipEvent_t es_ev = nullptr;         // behind that copy
    bool es_pending = false;
    int64_t es_nominal = 0;
    int32_t es_E = 0;                   // update_epochs of the pending update
    bool es_last_on = false;            // the last update ran with a target
    EarlyStopHost es_last{};            // its outcome, once resolved
    int64_t epochs_total = 0;           // epochs applied by all updates so far

    // statistics snapshot (ppo_stats_snapshot / ppo_stats_snapshot_read): everything ppo_read_stats decodes, copied asynchronously into ONE pinned block
    // behind the work enqueued so far; the reader waits for the snapshot's event only, so a host may enqueue the next iteration before it reads
    struct StatsSnap* snap = nullptr;   // [2]: a host that runs one iteration ahead takes snapshot k + 1 before it reads snapshot k
    hipEvent_t snap_ev[2] = { nullptr, nullptr };
    int snap_oldest = 0, snap_count = 0; // FIFO of pending snapshots

    // profiling: (start, stop) event pairs per instrumented launch
    uint32_t profiling = 0;         // bit k set: time launches of kind k
    struct Span { hipEvent_t a, b; int kind; };
    std::vector<Span> spans;
    std::vector<hipEvent_t> event_pool;
};

enum { PROF_FWD_BWD = 0, PROF_GAE, PROF_ROLLOUT, PROF_OPT, PROF_REDUCE, PROF_ALLREDUCE, PROF_KINDS_ };

struct ProfScope {
    ppo_ctx* c;
    hipEvent_t a = nullptr, b = nullptr;
    int kind;
    static hipEvent_t get(ppo_ctx* c) {
        if (!c->event_pool.empty()) { hipEvent_t e = c->event_pool.back(); c->event_pool.pop_back(); return e; }
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) != hipSuccess) return nullptr;
        return e;
    }
    ProfScope(ppo_ctx* ctx, int k, bool sampled_in = true) : c(ctx), kind(k) {
        if (!(c->profiling & (1u << kind)) || !sampled_in) return;
        a = get(c); b = get(c);
        if (a) (void)hipEventRecord(a, c->stream);
    }
    ~ProfScope() {
        if (!a || !b) return;
        (void)hipEventRecord(b, c->stream);
        c->spans.push_back({ a, b, kind });
    }
};

static thread_local std::string g_create_error;

// Every entry point that allocates, creates events or launches does so on the CONTEXT's device and leaves the caller's current device as it
// found it (a host that drives several contexts from one thread, or shares the thread with another HIP user such as PyTorch).
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    explicit DeviceGuard(const ppo_ctx* c) {
        if (!c) return;
        if (hipGetDevice(&prev) == hipSuccess && prev != c->cfg.device) switched = hipSetDevice(c->cfg.device) == hipSuccess;
    }
    ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
};

static ppo_status fail(ppo_ctx* ctx, ppo_status code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf; else g_create_error = buf;
    return code;
}

#define HIPCHK(ctx, call)                                                                                                   \
    do {                                                                                                                    \
        hipError_t e_ = (call);                                                                                             \
        if (e_ != hipSuccess) return fail(ctx, PPO_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)
#define NEED(ctx, cond, msg)                                        \
    do {                                                            \
        if (!(cond)) return fail(ctx, PPO_ERR_INVALID, "%s", msg);  \
    } while (0)

template <class Tp>
static hipError_t dalloc(ppo_ctx* c, Tp** p, size_t count, bool zero = true) {
    void* q = nullptr;
    const size_t bytes = std::max<size_t>(count * sizeof(Tp), 16);
    hipError_t e = hipMalloc(&q, bytes);
    if (e != hipSuccess) return e;
    c->allocs.push_back(q);
    if (zero) { e = hipMemset(q, 0, bytes); if (e != hipSuccess) return e; }
    *p = static_cast<Tp*>(q);
    return hipSuccess;
}
template <class Tp>
static hipError_t dalloc_buf(ppo_ctx* c, int which, size_t count) {
    Tp* p = nullptr;
    hipError_t e = dalloc(c, &p, count);
    c->buf[which] = p;
    c->buf_bytes[which] = count * sizeof(Tp);
    return e;
}
template <class Tp>
static Tp* B_(ppo_ctx* c, int which) { return static_cast<Tp*>(c->buf[which]); }

// DevEventList's life cycle.  Every step but events_read only enqueues or allocates: ppo_dev_observe, which must not wait, goes through the first three.
// Each piece is made once, so a call repeated after a failed allocation completes the list.  The counter is cleared in stream order (events_clear), not here.
static ppo_status events_reserve(ppo_ctx* c, DevEventList& l, int64_t cap) {
    if (l.cap > 0) return PPO_OK;
    if (!l.ev) HIPCHK(c, hipEventCreateWithFlags(&l.ev, hipEventDisableTiming));
    if (!l.count_h) {
        HIPCHK(c, hipHostMalloc(reinterpret_cast<void**>(&l.count_h), 4 * sizeof(int32_t), hipHostMallocDefault));
        l.count_h[0] = 0;
    }
    if (!l.count) HIPCHK(c, dalloc(c, &l.count, 4, false));
    if (!l.index) HIPCHK(c, dalloc(c, &l.index, (size_t)cap, false));
    if (!l.value) HIPCHK(c, dalloc(c, &l.value, (size_t)cap, false));
    l.cap = cap;
    return PPO_OK;
}
static ppo_status events_clear(ppo_ctx* c, DevEventList& l) {
    l.closed = false;
    HIPCHK(c, hipMemsetAsync(l.count, 0, sizeof(int32_t), c->stream));
    return PPO_OK;
}
template <class FoldArgs>   // DevFoldArgs, EnvFoldArgs, FusedFoldArgs
static void events_sink(const DevEventList& l, FoldArgs& f) { f.ev_count = l.count; f.ev_index = l.index; f.ev_value = l.value; f.ev_cap = l.cap; }
static ppo_status events_close(ppo_ctx* c, DevEventList& l) {
    HIPCHK(c, hipMemcpyAsync(l.count_h, l.count, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipEventRecord(l.ev, c->stream));
    l.closed = true;
    l.fetched = false;
    return PPO_OK;
}
// The array rules of ppo_host_truncations (trunc_events.hpp: copy_events_out).  A list that is not closed holds no event of the last rollout.
static ppo_status events_read(ppo_ctx* c, DevEventList& l, const char* what, int64_t* count, int32_t* index_h, float* value_h, int64_t cap) {
    if (!l.closed) {
        l.idx.clear();
        l.val.clear();
    } else if (!l.fetched) {   // on the device, in the order the workgroups got there
        DeviceGuard dev_guard(c);
        HIPCHK(c, hipEventSynchronize(l.ev));
        const int64_t n = clamp_event_count(l.count_h[0], l.cap);
        std::vector<int32_t> ix((size_t)n);
        std::vector<float> va((size_t)n);
        if (n > 0) {
            HIPCHK(c, hipMemcpy(ix.data(), l.index, (size_t)n * 4, hipMemcpyDeviceToHost));
            HIPCHK(c, hipMemcpy(va.data(), l.value, (size_t)n * 4, hipMemcpyDeviceToHost));
        }
        sort_events(ix, va, l.idx, l.val);
        l.fetched = true;
    }
    if (!copy_events_out(l.idx, l.val, count, index_h, value_h, cap))
        return fail(c, PPO_ERR_INVALID, "%s: room for %lld events, the last rollout had %lld", what, (long long)cap, (long long)l.idx.size());
    return PPO_OK;
}
static void events_release(DevEventList& l) {
    if (l.count_h) (void)hipHostFree(l.count_h);
    if (l.ev) (void)hipEventDestroy(l.ev);
}

// ---------------------------------------------------------------------------------------------------------
// host helpers
// ---------------------------------------------------------------------------------------------------------
namespace {
struct Mt19937 {
    uint32_t mt[624];
    int idx;
    explicit Mt19937(uint32_t s) {
        mt[0] = s;
        for (int i = 1; i < 624; i++) mt[i] = 1812433253u * (mt[i - 1] ^ (mt[i - 1] >> 30)) + (uint32_t)i;
        idx = 624;
    }
    uint32_t next() {
        if (idx >= 624) {
            for (int i = 0; i < 624; i++) {
                const uint32_t y = (mt[i] & 0x80000000u) | (mt[(i + 1) % 624] & 0x7fffffffu);
                mt[i] = mt[(i + 397) % 624] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
            }
            idx = 0;
        }
        uint32_t y = mt[idx++];
        y ^= y >> 11; y ^= (y << 7) & 0x9d2c5680u; y ^= (y << 15) & 0xefc60000u; y ^= y >> 18;
        return y;
    }
};
}  // namespace

// std::mt19937(seed) + std::uniform_real_distribution<float>(-0.05f, 0.05f): reference CartPole.h:28-29, CartPole.cpp:3-4,96-100.
// libstdc++'s generate_canonical<float,24> consumes one 32-bit draw: float(u)/2^32, clamped below 1; then *(b-a)+a.
extern "C" ppo_status ppo_cartpole_reset_stream_h(int64_t seed, int64_t n_resets, float* out_h) {
    if (!out_h || n_resets < 0) return PPO_ERR_INVALID;
    Mt19937 g((uint32_t)seed);
    const float a = -0.05f, b = 0.05f;
    for (int64_t i = 0; i < n_resets * 4; i++) {
        float r = (float)g.next() / 4294967296.0f;
        if (r >= 1.0f) r = std::nextafter(1.0f, 0.0f);
        out_h[i] = r * (b - a) + a;
    }
    return PPO_OK;
}

static ppo_status ensure_reset_table(ppo_ctx* c, int64_t need) {
    if (c->cfg.env_kind != PPO_ENV_CARTPOLE) return PPO_OK;
    if (need <= c->reset_cap) return PPO_OK;
    int64_t cap = std::max<int64_t>(c->reset_cap, 1024);
    while (cap < need) cap *= 2;
    NEED(c, cap < (1ll << 28), "reset table would exceed 2^28 entries");
    std::vector<float> h((size_t)cap * 4);
    ppo_cartpole_reset_stream_h(c->cfg.seed, cap, h.data());
    float* d = nullptr;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&d), (size_t)cap * 4 * sizeof(float)));
    HIPCHK(c, hipMemcpy(d, h.data(), (size_t)cap * 4 * sizeof(float), hipMemcpyHostToDevice));
    if (c->reset_table) {
        c->allocs.erase(std::remove(c->allocs.begin(), c->allocs.end(), (void*)c->reset_table), c->allocs.end());
        (void)hipFree(c->reset_table);
    }
    c->allocs.push_back(d);
    c->reset_table = d;
    c->reset_cap = (int)cap;
    return PPO_OK;
}

// Direct exchange: a kernel whose bounded wait for a peer ran out has summed only the shares that arrived and marked the communicator dead.  The
// stream is idle here (every caller has just synchronised it): turn the flag into an error instead of letting diverged replicas train on.
static ppo_status comm_health(ppo_ctx* c) {
    if (!c->xchg || !c->xchg->timeout_flag) return PPO_OK;
    int32_t f = 0;
    HIPCHK(c, hipMemcpy(&f, c->xchg->timeout_flag, sizeof f, hipMemcpyDeviceToHost));
    if (f != 0)
        return fail(c, PPO_ERR_COMM, "direct exchange: an all-reduce gave up waiting for a peer after %.1f s; its sums were incomplete, the replicas have "
                                     "diverged and the communicator is dead (every later all-reduce returns at once)", c->xchg->wait_seconds);
    return PPO_OK;
}

// ---------------------------------------------------------------------------------------------------------
// lifecycle
// ---------------------------------------------------------------------------------------------------------
extern "C" int32_t ppo_abi_version(void) { return PPO_ABI_VERSION; }

extern "C" const char* ppo_last_error(const ppo_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

extern "C" void ppo_ctx_destroy(ppo_ctx* c) {
    if (!c) return;
    // teardown is best effort: nothing useful can be done with a failing release, and there is no caller to tell
    (void)hipSetDevice(c->cfg.device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->comm && rccl::CommDestroy) rccl::CommDestroy(c->comm);
    if (c->lg_ready) (void)hipEventDestroy(c->lg_ready);
    if (c->xchg) {
        for (int r = 0; r < 8; r++) if (c->xchg->opened[r]) (void)hipIpcCloseMemHandle(c->xchg->peer[r]);
        if (c->xchg->own) (void)hipFree(c->xchg->own);
    }
    for (auto& sp : c->spans) { (void)hipEventDestroy(sp.a); (void)hipEventDestroy(sp.b); }
    for (hipEvent_t e : c->event_pool) (void)hipEventDestroy(e);
    if (c->gen) { delete c->gen; c->gen = nullptr; }
    for (void* p : c->allocs) (void)hipFree(p);
    if (c->adam_coefs_h) (void)hipHostFree(c->adam_coefs_h);
    if (c->host_stage) (void)hipHostFree(c->host_stage);
    if (c->host_act) (void)hipHostFree(c->host_act);
    for (auto& hg : c->host_grp) if (hg.ev) (void)hipEventDestroy(hg.ev);
    if (c->trunc_h) (void)hipHostFree(c->trunc_h);
    if (c->trunc_dev) (void)hipFree(c->trunc_dev);
    if (c->trunc_ev) (void)hipEventDestroy(c->trunc_ev);
    if (c->dev_ev_in) (void)hipEventDestroy(c->dev_ev_in);
    if (c->dev_ev_out) (void)hipEventDestroy(c->dev_ev_out);
    for (DevEventList* l : { &c->dev_events[0], &c->dev_events[1], &c->env_events }) events_release(*l);
    if (c->wr_host) (void)hipHostFree(c->wr_host);
    if (c->snap) (void)hipHostFree(c->snap);
    if (c->es_host) (void)hipHostFree(c->es_host);
    if (c->es_ev) (void)hipEventDestroy(c->es_ev);
    for (hipEvent_t e : c->snap_ev) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->coef_copied) if (e) (void)hipEventDestroy(e);
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    if (c->ev_join) (void)hipEventDestroy(c->ev_join);
    if (c->ev_gather) (void)hipEventDestroy(c->ev_gather);
    if (c->stream2) (void)hipStreamDestroy(c->stream2);
    if (c->wr_stream) { (void)hipStreamSynchronize(c->wr_stream); (void)hipStreamDestroy(c->wr_stream); }
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

// The pinned staging block of caller-stepped envs (ppo_ctx::host_stage): the byte offset of each area and the block's size, written down here only
struct HostStage { size_t obs, rew, done, fin_len, fin_rew, mask, bytes; };
static HostStage host_stage_layout(size_t N, size_t O, size_t A) {
    HostStage l{};   // obs f32 [N,O] at 0, then four 4-byte [N] columns, then the mask u8 [N,A]
    l.rew = l.obs + N * O * 4; l.done = l.rew + N * 4; l.fin_len = l.done + N * 4; l.fin_rew = l.fin_len + N * 4; l.mask = l.fin_rew + N * 4;
    l.bytes = (l.mask + N * A + 15) / 16 * 16;
    return l;
}
static HostStage host_stage_layout(const ppo_ctx* c) { return host_stage_layout((size_t)c->N, (size_t)c->O, (size_t)c->A); }

extern "C" ppo_status ppo_ctx_create(const ppo_config* cfg, ppo_ctx** out) {
    if (!cfg || !out) return fail(nullptr, PPO_ERR_INVALID, "null argument");
    *out = nullptr;
    if (cfg->struct_size != (int32_t)sizeof(ppo_config)) return fail(nullptr, PPO_ERR_INVALID, "ppo_config.struct_size %d != %zu", cfg->struct_size, sizeof(ppo_config));
    // PPO_ENV_HOST: the caller's envs (ppo_host_*).  The reference's network (2 x 64, f32) at the observation widths the reference-shape kernels are built
    // for runs on them; every other network on the generic engine, with PPO_ENV_SYNTHETIC's limits
    const bool host_env = cfg->env_kind == PPO_ENV_HOST;
    const bool gauss = cfg->dist_kind == PPO_DIST_GAUSSIAN;   // diagonal-Gaussian policies: always the generic engine (kernels_gauss.hip)
    // PPO_KERNEL_CAT_FUSED: always the generic engine's layout, also at the observation widths of the reference-shape kernels (checked below)
    const bool cat_fused = (cfg->kernel_flags & PPO_KERNEL_CAT_FUSED) != 0;
    const bool host_ref = host_env && !gauss && !cat_fused && cfg->hidden == PPO_HIDDEN && cfg->n_hidden == 2 && cfg->compute_dtype == PPO_DTYPE_F32 &&
                          (cfg->obs_size == 2 || cfg->obs_size == 4 || cfg->obs_size == 8);
    // a device env of the fused 2 x 64 kernel families (gauss_fused.hpp: FusedEnvInfo): the network lives in the generic engine's layout (GenericCtx), as a
    // PPO_ENV_HOST context with the family's flag does, and only the rollout differs (gauss_rollout_kernel / cat_rollout_kernel)
    const FusedEnvInfo* env = fused_env_info(cfg->env_kind);
    const bool gauss_env = env && env->family == FUSED_GAUSS, cat_env = env && env->family == FUSED_CAT;
    // PPO_KERNEL_ENV_GENERIC on CartPole / MountainCar: the network lives in the generic engine's layout, with PPO_ENV_SYNTHETIC's limits (the flag anywhere
    // else is refused below, behind the checks of env_kind, dist_kind, compute_dtype and of the flag word itself)
    const bool env_generic = (cfg->kernel_flags & PPO_KERNEL_ENV_GENERIC) != 0 && (cfg->env_kind == PPO_ENV_CARTPOLE || cfg->env_kind == PPO_ENV_MOUNTAINCAR);
    const bool generic = cfg->env_kind == PPO_ENV_SYNTHETIC || (host_env && !host_ref) || gauss_env || cat_env || env_generic;
    if (!generic && (cfg->hidden != PPO_HIDDEN || cfg->n_hidden != 2))
        return fail(nullptr, PPO_ERR_UNSUPPORTED, "only the reference architecture (2 hidden layers of 64, Agent.cpp:25-59) is built for the reference's "
                    "environments; got %d x %d (other shapes run with env_kind = PPO_ENV_SYNTHETIC)", cfg->n_hidden, cfg->hidden);
    if (generic && !gauss_env && !cat_env && (cfg->hidden < 1 || cfg->hidden > 2048 || cfg->n_hidden < 1 || cfg->n_hidden > GEN_MAX_LAYERS - 1 || cfg->obs_size < 1 || cfg->obs_size > 8192))
        return fail(nullptr, PPO_ERR_UNSUPPORTED, "generic network out of range: hidden %d (1..2048), n_hidden %d (1..%d), obs %d (1..8192)", cfg->hidden,
                    cfg->n_hidden, GEN_MAX_LAYERS - 1, cfg->obs_size);
    if (cfg->env_kind != PPO_ENV_CARTPOLE && cfg->env_kind != PPO_ENV_MOUNTAINCAR && cfg->env_kind != PPO_ENV_SYNTHETIC && cfg->env_kind != PPO_ENV_HOST && !gauss_env && !cat_env)
        return fail(nullptr, PPO_ERR_INVALID, "unknown env_kind %d", cfg->env_kind);
    if (cfg->dist_kind != PPO_DIST_CATEGORICAL && cfg->dist_kind != PPO_DIST_MASKED && !gauss) return fail(nullptr, PPO_ERR_INVALID, "unknown dist_kind %d", cfg->dist_kind);
    if (cfg->compute_dtype != PPO_DTYPE_F32 && cfg->compute_dtype != PPO_DTYPE_BF16) return fail(nullptr, PPO_ERR_INVALID, "unknown compute_dtype %d", cfg->compute_dtype);
    constexpr int32_t known_flags = PPO_KERNEL_ROLLOUT_VECTOR | PPO_KERNEL_UPDATE_VECTOR | PPO_KERNEL_UPDATE_ONE_WAVE | PPO_KERNEL_COMM_SELFTEST | PPO_KERNEL_GENERIC_CLASSIC |
                                  PPO_KERNEL_GENERIC_SPLIT_HEAD | PPO_KERNEL_GAUSS_FUSED | PPO_KERNEL_SEPARATE_LAUNCHES | PPO_KERNEL_CAT_FUSED | PPO_KERNEL_ENV_GENERIC |
                                  PPO_KERNEL_ENV_CUT_STATE | PPO_KERNEL_ENV_REWARD_NORM;
    // PPO_KERNEL_ENV_CUT_STATE: a device env of the fused 2 x 64 families (a row of fused_env_rows), next to that env's own family flag (checked in the env's
    // block below), or a refusal that names the flag.  In front of PPO_KERNEL_ENV_GENERIC's block, so that the two flags together are answered here
    if (cfg->kernel_flags & PPO_KERNEL_ENV_CUT_STATE) {
        if (cfg->kernel_flags & ~known_flags) return fail(nullptr, PPO_ERR_INVALID, "unknown bits in kernel_flags 0x%x", cfg->kernel_flags);
        if (cfg->kernel_flags & PPO_KERNEL_ENV_GENERIC)
            return fail(nullptr, PPO_ERR_UNSUPPORTED, "PPO_KERNEL_ENV_CUT_STATE excludes PPO_KERNEL_ENV_GENERIC: the cut-off state is kept by the one-launch rollouts of "
                        "the fused 2 x 64 families, and CartPole / MountainCar on the generic engine run neither");
        if (!env)
            return fail(nullptr, PPO_ERR_UNSUPPORTED, "PPO_KERNEL_ENV_CUT_STATE serves the device envs of the fused 2 x 64 families only (%s; %s): their one-launch "
                        "rollouts keep the state a time limit cut an episode off in; CartPole and MountainCar fold from PPO_BUF_OBS without it, PPO_ENV_SYNTHETIC "
                        "has no last observation and PPO_ENV_HOST passes its own (ppo_host_observe_truncated); got env_kind %d",
                        fused_env_names(FUSED_GAUSS), fused_env_names(FUSED_CAT), cfg->env_kind);
    }
    // PPO_KERNEL_ENV_REWARD_NORM: accepted exactly where PPO_KERNEL_ENV_CUT_STATE is (and beside it), or a refusal that names the flag
    if (cfg->kernel_flags & PPO_KERNEL_ENV_REWARD_NORM) {
        if (cfg->kernel_flags & ~known_flags) return fail(nullptr, PPO_ERR_INVALID, "unknown bits in kernel_flags 0x%x", cfg->kernel_flags);
        if (cfg->kernel_flags & PPO_KERNEL_ENV_GENERIC)
            return fail(nullptr, PPO_ERR_UNSUPPORTED, "PPO_KERNEL_ENV_REWARD_NORM excludes PPO_KERNEL_ENV_GENERIC: the rewards are normalised behind the one-launch "
                        "rollouts of the fused 2 x 64 families, and CartPole / MountainCar on the generic engine run neither");
        if (!env)
            return fail(nullptr, PPO_ERR_UNSUPPORTED, "PPO_KERNEL_ENV_REWARD_NORM serves the device envs of the fused 2 x 64 families only (%s; %s): it opens "
                        "ppo_reward_norm_* on their one-launch rollouts; CartPole, MountainCar and PPO_ENV_SYNTHETIC pay rewards of unit scale and "
                        "PPO_ENV_HOST has the three calls without a flag; got env_kind %d",
                        fused_env_names(FUSED_GAUSS), fused_env_names(FUSED_CAT), cfg->env_kind);
    }
    // PPO_KERNEL_ENV_GENERIC: CartPole / MountainCar with a categorical policy and neither flag of the fused 2 x 64 family, or a refusal that names the flag --
    // never another engine in its place.  In front of the envs' own blocks, so that the flag on one of them is answered here
    if (cfg->kernel_flags & PPO_KERNEL_ENV_GENERIC) {
        if (cfg->kernel_flags & ~known_flags) return fail(nullptr, PPO_ERR_INVALID, "unknown bits in kernel_flags 0x%x", cfg->kernel_flags);
        if (!env_generic)
            return fail(nullptr, PPO_ERR_UNSUPPORTED, "PPO_KERNEL_ENV_GENERIC serves env_kind = PPO_ENV_CARTPOLE and PPO_ENV_MOUNTAINCAR only (the other device envs "
                        "run on their own kernel families, PPO_ENV_SYNTHETIC and PPO_ENV_HOST are on the generic engine without it); got env_kind %d", cfg->env_kind);
        if (cfg->kernel_flags & (PPO_KERNEL_GAUSS_FUSED | PPO_KERNEL_CAT_FUSED))
            return fail(nullptr, PPO_ERR_UNSUPPORTED, "PPO_KERNEL_ENV_GENERIC excludes PPO_KERNEL_GAUSS_FUSED and PPO_KERNEL_CAT_FUSED: those flags name the fused 2 x 64 "
                        "kernel family, this one the generic engine; a context runs on one of them");
        if (gauss)
            return fail(nullptr, PPO_ERR_UNSUPPORTED, "PPO_KERNEL_ENV_GENERIC serves dist_kind = PPO_DIST_CATEGORICAL and PPO_DIST_MASKED only: CartPole and MountainCar take "
                        "discrete actions; got PPO_DIST_GAUSSIAN");
    }
    if (env && cfg->obs_size == env->obs) {   // accepted in exactly the forms ppo_hip.h states; a wrong obs_size first, with the reference's message (below)
        const bool g = env->family == FUSED_GAUSS;
        const char* kernels = g ? "fused Gaussian" : "fused categorical";
        if (!(env->dist_mask >> cfg->dist_kind & 1))
            return fail(nullptr, PPO_ERR_UNSUPPORTED, "env_kind = %s takes %s: it is built for dist_kind = %s; got dist_kind %d", env->name, env->text.takes,
                        g ? "PPO_DIST_GAUSSIAN" : (env->dist_mask >> PPO_DIST_MASKED & 1 ? "PPO_DIST_MASKED and PPO_DIST_CATEGORICAL" : "PPO_DIST_CATEGORICAL"),
                        cfg->dist_kind);
        if (cfg->n_heads != 1 || cfg->head_dims[0] != env->actions)
            return fail(nullptr, PPO_ERR_UNSUPPORTED, "env_kind = %s has %s: n_heads = 1 and head_dims[0] = %d; got n_heads = %d, head_dims[0] = %d", env->name,
                        env->text.head, env->actions, cfg->n_heads, cfg->head_dims[0]);
        if (cfg->hidden != 64 || cfg->n_hidden != 2)
            return fail(nullptr, PPO_ERR_UNSUPPORTED, "env_kind = %s is built for the 2 x 64 network (hidden = 64, n_hidden = 2) of the %s kernels; got %d x %d",
                        env->name, kernels, cfg->n_hidden, cfg->hidden);
        if (cfg->compute_dtype != PPO_DTYPE_F32)
            return fail(nullptr, PPO_ERR_UNSUPPORTED, "env_kind = %s is built for compute_dtype = PPO_DTYPE_F32; bf16 storage is not", env->name);
        if (!(cfg->kernel_flags & (g ? PPO_KERNEL_GAUSS_FUSED : PPO_KERNEL_CAT_FUSED)))
            return fail(nullptr, PPO_ERR_UNSUPPORTED, "env_kind = %s needs %s in kernel_flags: its rollout exists on the %s kernels only, and the flag is never "
                        "implied (no other engine serves in its place)", env->name, g ? "PPO_KERNEL_GAUSS_FUSED" : "PPO_KERNEL_CAT_FUSED", kernels);
        if (cfg->max_episode_steps < 1 || (env->max_steps && cfg->max_episode_steps > env->max_steps))
            return env->max_steps ? fail(nullptr, PPO_ERR_UNSUPPORTED, "env_kind = %s is built for 1 <= max_episode_steps <= %d (%s); got %d", env->name,
                                         env->max_steps, env->text.steps_why, cfg->max_episode_steps)
                                  : fail(nullptr, PPO_ERR_UNSUPPORTED, "env_kind = %s is built for max_episode_steps >= 1 (%s); got %d", env->name, env->text.steps_why,
                                         cfg->max_episode_steps);
    }
    if (gauss && !host_env && !gauss_env)
        return fail(nullptr, PPO_ERR_UNSUPPORTED, "dist_kind = PPO_DIST_GAUSSIAN serves caller-stepped environments (env_kind = PPO_ENV_HOST), %s: CartPole, MountainCar "
                    "and the synthetic env take discrete actions; got env_kind %d", fused_env_names(FUSED_GAUSS), cfg->env_kind);
    if (gauss && cfg->compute_dtype != PPO_DTYPE_F32)
        return fail(nullptr, PPO_ERR_UNSUPPORTED, "dist_kind = PPO_DIST_GAUSSIAN is built for compute_dtype = PPO_DTYPE_F32; bf16 storage is not");
    if (gauss && cfg->n_heads != 1)
        return fail(nullptr, PPO_ERR_UNSUPPORTED, "dist_kind = PPO_DIST_GAUSSIAN takes n_heads = 1 with head_dims[0] = the action dimension D; got n_heads = %d", cfg->n_heads);
    if (cfg->kernel_flags & ~known_flags) return fail(nullptr, PPO_ERR_INVALID, "unknown bits in kernel_flags 0x%x", cfg->kernel_flags);
    // PPO_KERNEL_CAT_FUSED: the one form kernels_gauss_fused.hip's categorical kernels are built for, or a refusal -- never another engine in its place
    if (cat_fused) {
        if (cfg->kernel_flags & PPO_KERNEL_GAUSS_FUSED)
            return fail(nullptr, PPO_ERR_UNSUPPORTED, "PPO_KERNEL_CAT_FUSED and PPO_KERNEL_GAUSS_FUSED exclude each other: a policy is categorical or Gaussian");
        if (gauss)
            return fail(nullptr, PPO_ERR_UNSUPPORTED, "PPO_KERNEL_CAT_FUSED serves dist_kind = PPO_DIST_CATEGORICAL and PPO_DIST_MASKED only; this context's policy is "
                        "PPO_DIST_GAUSSIAN (its twin is PPO_KERNEL_GAUSS_FUSED)");
        if (!host_env && !cat_env)
            return fail(nullptr, PPO_ERR_UNSUPPORTED, "PPO_KERNEL_CAT_FUSED serves caller-stepped environments (env_kind = PPO_ENV_HOST), %s only; got env_kind %d",
                        fused_env_names(FUSED_CAT), cfg->env_kind);
        if (cfg->hidden != 64) return fail(nullptr, PPO_ERR_UNSUPPORTED, "PPO_KERNEL_CAT_FUSED is built for hidden = 64; got hidden = %d", cfg->hidden);
        if (cfg->n_hidden != 2) return fail(nullptr, PPO_ERR_UNSUPPORTED, "PPO_KERNEL_CAT_FUSED is built for n_hidden = 2; got n_hidden = %d", cfg->n_hidden);
        if (cfg->compute_dtype != PPO_DTYPE_F32)
            return fail(nullptr, PPO_ERR_UNSUPPORTED, "PPO_KERNEL_CAT_FUSED is built for compute_dtype = PPO_DTYPE_F32; bf16 storage is not");
        if (cfg->obs_size < 1 || cfg->obs_size > GAUSS_FUSED_MAX_OBS)
            return fail(nullptr, PPO_ERR_UNSUPPORTED, "PPO_KERNEL_CAT_FUSED is built for 1 <= obs_size <= %d; got obs_size = %d", GAUSS_FUSED_MAX_OBS, cfg->obs_size);
    }
    if (cfg->compute_dtype == PPO_DTYPE_BF16 && !generic)
        return fail(nullptr, PPO_ERR_UNSUPPORTED, "compute_dtype = PPO_DTYPE_BF16 applies to networks whose layers are GEMMs (env_kind = PPO_ENV_SYNTHETIC); the reference's "
                    "2 x 64 networks always compute in f32");
    const int env_obs = env ? env->obs : (cfg->env_kind == PPO_ENV_CARTPOLE ? 4 : (cfg->env_kind == PPO_ENV_MOUNTAINCAR ? 2 : cfg->obs_size));   // host / synthetic: no check
    if (cfg->obs_size != env_obs) {
        // the reference's runtime check in initEnvs (PPO_Discrete.cpp:370-375), same wording
        return fail(nullptr, PPO_ERR_INVALID,
                    "The environment returned an observation of size %d, but your config defined the expected observation size to be %d.\n"
                    "Have you properly defined your PPOConfig.toml file for your environment?", env_obs, cfg->obs_size);
    }
    if (cfg->n_heads < 1 || cfg->n_heads > PPO_MAX_HEADS) return fail(nullptr, PPO_ERR_INVALID, "n_heads must be in [1,%d]", PPO_MAX_HEADS);
    int A = 0;
    for (int h = 0; h < cfg->n_heads; h++) {
        if (cfg->head_dims[h] < 1) return fail(nullptr, PPO_ERR_INVALID, "head_dims[%d] < 1", h);
        A += cfg->head_dims[h];
    }
    if (A > PPO_MAX_ACT) return fail(nullptr, PPO_ERR_UNSUPPORTED, "sum(head_dims) = %d exceeds %d", A, PPO_MAX_ACT);
    // PPO_KERNEL_GAUSS_FUSED: the one shape kernels_gauss_fused.hip is built for, or a refusal -- never the generic engine in its place
    const bool gauss_fused = (cfg->kernel_flags & PPO_KERNEL_GAUSS_FUSED) != 0;
    if (gauss_fused) {
        if (!gauss)
            return fail(nullptr, PPO_ERR_UNSUPPORTED, "PPO_KERNEL_GAUSS_FUSED serves dist_kind = PPO_DIST_GAUSSIAN only; this context's policy is categorical (dist_kind %d)",
                        cfg->dist_kind);
        if (cfg->hidden != 64) return fail(nullptr, PPO_ERR_UNSUPPORTED, "PPO_KERNEL_GAUSS_FUSED is built for hidden = 64; got hidden = %d", cfg->hidden);
        if (cfg->n_hidden != 2) return fail(nullptr, PPO_ERR_UNSUPPORTED, "PPO_KERNEL_GAUSS_FUSED is built for n_hidden = 2; got n_hidden = %d", cfg->n_hidden);
        if (cfg->obs_size > GAUSS_FUSED_MAX_OBS)
            return fail(nullptr, PPO_ERR_UNSUPPORTED, "PPO_KERNEL_GAUSS_FUSED is built for obs_size <= %d; got obs_size = %d", GAUSS_FUSED_MAX_OBS, cfg->obs_size);
        if (!gauss_fused_serves_shape(cfg->obs_size, cfg->hidden, cfg->n_hidden, A))
            return fail(nullptr, PPO_ERR_UNSUPPORTED, "PPO_KERNEL_GAUSS_FUSED is built for 1 <= D <= %d and 1 <= obs_size <= %d; got D = %d, obs_size = %d", PPO_MAX_ACT,
                        GAUSS_FUSED_MAX_OBS, A, cfg->obs_size);
    }
    if (cat_fused && !cat_fused_serves_shape(cfg->obs_size, cfg->hidden, cfg->n_hidden, A))   // the head list's limits are the ABI's own, checked above
        return fail(nullptr, PPO_ERR_UNSUPPORTED, "PPO_KERNEL_CAT_FUSED is built for sum(head_dims) <= %d and 1 <= obs_size <= %d; got %d, obs_size = %d", PPO_MAX_ACT,
                    GAUSS_FUSED_MAX_OBS, A, cfg->obs_size);
    if (cfg->num_envs < 1 || cfg->num_steps < 1 || cfg->num_minibatches < 1 || cfg->update_epochs < 1)
        return fail(nullptr, PPO_ERR_INVALID, "num_envs, num_steps, num_minibatches, update_epochs must be >= 1");
    const int64_t B = (int64_t)cfg->num_envs * cfg->num_steps;
    if (B / cfg->num_minibatches < 1) return fail(nullptr, PPO_ERR_INVALID, "minibatch_size = batch/num_minibatches is 0");
    if (B >= (1ll << 31)) return fail(nullptr, PPO_ERR_UNSUPPORTED, "batch of %lld rows exceeds int32 indexing", (long long)B);

    int caller_device = -1;
    (void)hipGetDevice(&caller_device);
    struct Restore { int d; ~Restore() { if (d >= 0) (void)hipSetDevice(d); } } restore_device{ caller_device };
    hipError_t e = hipSetDevice(cfg->device);
    if (e != hipSuccess) return fail(nullptr, PPO_ERR_HIP, "hipSetDevice(%d): %s", cfg->device, hipGetErrorString(e));
    ppo_ctx* c = new ppo_ctx();
    c->cfg = *cfg;
    c->env = env;
    if (c->cfg.global_num_envs <= 0) c->cfg.global_num_envs = cfg->num_envs;
    c->L = make_layout(cfg->obs_size, cfg->n_heads, cfg->head_dims);
    if (generic) {
        c->gen = new GenericCtx();
        c->gen->L = make_gen_layout(cfg->obs_size, cfg->hidden, cfg->n_hidden, cfg->n_heads, cfg->head_dims, gauss);
        // the shared code sizes the flat parameter / gradient / moment buffers from L.P; the 2 x 64 offsets in L are not used
        c->L.P = c->gen->L.P;
        c->L.n_tensors = c->gen->L.n_tensors;
        c->L.net_size[0] = c->L.net_size[1] = 1;   // no per-workgroup gradient slabs on this path
    }
    c->hp = LossParams{ cfg->clip_coef, cfg->ent_coef, cfg->vf_coef, cfg->norm_adv, cfg->clip_vloss, cfg->dist_kind };
    c->T = cfg->num_steps; c->N = cfg->num_envs; c->O = cfg->obs_size; c->H = cfg->n_heads; c->A = A;
    c->B = B;
    c->MB = B / cfg->num_minibatches;                 // int division, PPO_Discrete.cpp:247
    c->n_mb = (int)((B + c->MB - 1) / c->MB);          // a ragged tail is an extra short minibatch (:573-576)
    c->steps_per_update = cfg->update_epochs * c->n_mb;
    c->lr = (double)cfg->learning_rate;                // AdamWOptions(m_learning_rate): double(float lr), :76-78
    const int64_t global_B = c->cfg.global_num_envs * (int64_t)cfg->num_steps;
    c->num_updates_total = cfg->total_timesteps > 0 ? cfg->total_timesteps / global_B : 0;  // :496

#define CK(call)                                                                                         \
    do {                                                                                                 \
        hipError_t e2 = (call);                                                                          \
        if (e2 != hipSuccess) {                                                                          \
            fail(nullptr, PPO_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e2));                    \
            ppo_ctx_destroy(c);                                                                          \
            return PPO_ERR_HIP;                                                                          \
        }                                                                                                \
    } while (0)
    CK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    const size_t TN = (size_t)c->T * c->N, N = c->N, P = c->L.P;
    CK(dalloc_buf<float>(c, PPO_BUF_OBS, TN * c->O));
    CK(dalloc_buf<int32_t>(c, PPO_BUF_ACTIONS, TN * (gauss ? A : c->H)));   // Gaussian: f32 [T,N,D] (the same 4-byte elements)
    CK(dalloc_buf<float>(c, PPO_BUF_LOGPROBS, TN));
    CK(dalloc_buf<float>(c, PPO_BUF_REWARDS, TN));
    CK(dalloc_buf<float>(c, PPO_BUF_DONES, TN));
    CK(dalloc_buf<float>(c, PPO_BUF_VALUES, TN));
    CK(dalloc_buf<uint8_t>(c, PPO_BUF_MASKS, TN * c->A));
    CK(dalloc_buf<float>(c, PPO_BUF_ADVANTAGES, TN));
    CK(dalloc_buf<float>(c, PPO_BUF_RETURNS, TN));
    CK(dalloc_buf<float>(c, PPO_BUF_NEXT_OBS, N * c->O));
    CK(dalloc_buf<int32_t>(c, PPO_BUF_NEXT_DONE, N));
    CK(dalloc_buf<float>(c, PPO_BUF_NEXT_VALUE, N));
    CK(dalloc_buf<float>(c, PPO_BUF_PARAMS, P));
    CK(dalloc_buf<float>(c, PPO_BUF_GRADS, P + 8));   // + loss sums that ride through the all-reduce when sharded
    c->buf_bytes[PPO_BUF_GRADS] = P * sizeof(float);
    CK(dalloc_buf<float>(c, PPO_BUF_EXP_AVG, P));
    CK(dalloc_buf<float>(c, PPO_BUF_EXP_AVG_SQ, P));
    CK(dalloc_buf<float>(c, PPO_BUF_ENV_STATE, N * c->O));
    CK(dalloc_buf<int32_t>(c, PPO_BUF_EP_LEN, N));
    CK(dalloc_buf<float>(c, PPO_BUF_EP_REW, N));
    CK(dalloc_buf<int32_t>(c, PPO_BUF_RESET_COUNT, N));
    CK(dalloc_buf<int32_t>(c, PPO_BUF_PERM, (size_t)cfg->update_epochs * B));
    CK(dalloc_buf<int32_t>(c, PPO_BUF_FIN_LEN, TN));
    CK(dalloc_buf<float>(c, PPO_BUF_FIN_REW, TN));
    CK(dalloc(c, &c->error_flag, 1));
    CK(dalloc(c, &c->wr_dev, 8));   // [0..2] running maxima, [4..6] what the host mirror holds
    CK(hipHostMalloc(reinterpret_cast<void**>(&c->wr_host), 4 * sizeof(uint32_t), hipHostMallocMapped));
    CK(hipHostGetDevicePointer(reinterpret_cast<void**>(&c->wr_host_dev), c->wr_host, 0));
    CK(hipStreamCreateWithFlags(&c->wr_stream, hipStreamNonBlocking));
    for (int i = 0; i < 4; i++) c->wr_host[i] = 0u;
    c->use_mfma = A <= 4;   // the matrix-core update kernel folds heads of up to 4 logits; wider policies (2 x 64 nets) run the vector kernel
    // ppo_config.kernel_flags (include/ppo_hip.h): the only switch between kernels; nothing is read from the environment
    if (cfg->kernel_flags & PPO_KERNEL_UPDATE_VECTOR) c->use_mfma = false;
    // the matrix-core update kernels (and their record packing) are built for the reference's observation widths 2 and 4; a caller-stepped env with 8
    // observations trains on the vector update kernel (fwd_bwd_kernel), which serves 2, 4 and 8
    if (!generic && c->O != 2 && c->O != 4) c->use_mfma = false;
    c->update_single_wave = (cfg->kernel_flags & PPO_KERNEL_UPDATE_ONE_WAVE) != 0;
    c->rollout_vector = (cfg->kernel_flags & PPO_KERNEL_ROLLOUT_VECTOR) != 0;
    c->separate_launches = (cfg->kernel_flags & PPO_KERNEL_SEPARATE_LAUNCHES) != 0;
    c->max_blocks_per_net = 512;
    const int Pmax = std::max(c->L.net_size[0], c->L.net_size[1]);
    CK(dalloc(c, &c->slab, (size_t)2 * c->max_blocks_per_net * Pmax));
    CK(dalloc(c, &c->stat_slab, (size_t)2 * c->max_blocks_per_net * 8));
    CK(dalloc(c, &c->loss_sums, 8));
    {   // [gstats | adv_stats] contiguous: a sharded update sends both in ONE all-reduce
        double* blk = nullptr;
        CK(dalloc(c, &blk, (size_t)PPO_GSTAT_DOUBLES + ((size_t)c->steps_per_update + 1) * PPO_ADV_PARTS * (sizeof(AdvStat) / sizeof(double))));
        c->gstats = blk;
        c->adv_stats = reinterpret_cast<AdvStat*>(blk + PPO_GSTAT_DOUBLES);
        CK(dalloc(c, &c->adv_norm, (size_t)c->steps_per_update + 1));
    }
    CK(dalloc(c, &c->adam_coefs, (size_t)c->steps_per_update + 1));
    CK(hipHostMalloc(reinterpret_cast<void**>(&c->adam_coefs_h), 2 * ((size_t)c->steps_per_update + 1) * sizeof(AdamCoef)));
    CK(hipHostMalloc(reinterpret_cast<void**>(&c->snap), 2 * sizeof(StatsSnap)));
    CK(hipEventCreateWithFlags(&c->snap_ev[0], hipEventDisableTiming));
    CK(hipEventCreateWithFlags(&c->snap_ev[1], hipEventDisableTiming));
    CK(hipEventCreateWithFlags(&c->coef_copied[0], hipEventDisableTiming));
    CK(hipEventCreateWithFlags(&c->coef_copied[1], hipEventDisableTiming));
    CK(dalloc(c, &c->step_stats, (size_t)c->steps_per_update + 1));
    CK(dalloc(c, &c->clipfrac_accum, 2));
    CK(dalloc(c, &c->norm2, (4 * GEN_MAX_LAYERS + 1) * GEN_NORM_PARTS));
    CK(dalloc(c, &c->fused_partial, (size_t)fused_opt_blocks(c->L) * 12));
    CK(dalloc(c, &c->ev_sums, PPO_EV_BLOCKS * 4));
    if (c->use_mfma && !generic) {
        CK(dalloc(c, &c->rec_critic, (size_t)B * 16));   // both nets' records of a sample side by side: one 64-byte sector (kernels_update_mfma.hip: pack_records_kernel)
        c->rec_actor = c->rec_critic + 8;
    }
    CK(dalloc(c, &c->row_counts, (size_t)c->T));
    CK(dalloc(c, &c->group_bits, (size_t)c->T * ((N + 63) / 64)));
    CK(dalloc(c, &c->ring, 1));
    CK(dalloc(c, &c->pair_tickets, 4));
    CK(dalloc(c, &c->scratch_obs, N * c->O));
    CK(dalloc(c, &c->stamps, 24));
    if (host_env) {
        c->host_env = true;
        c->host_stage_bytes = host_stage_layout(c).bytes;
        CK(hipHostMalloc(reinterpret_cast<void**>(&c->host_stage), c->host_stage_bytes, hipHostMallocMapped));
        CK(hipHostGetDevicePointer(reinterpret_cast<void**>(&c->host_stage_dev), c->host_stage, 0));
        std::memset(c->host_stage, 0, c->host_stage_bytes);
        CK(hipHostMalloc(reinterpret_cast<void**>(&c->host_act), std::max(N * c->H * sizeof(int64_t), gauss ? N * A * sizeof(float) : (size_t)0), hipHostMallocMapped));
        CK(hipHostGetDevicePointer(reinterpret_cast<void**>(&c->host_act_dev), c->host_act, 0));
        for (auto& hg : c->host_grp) CK(hipEventCreateWithFlags(&hg.ev, hipEventDisableTiming));
    }
    if (c->gen) {
        GenericCtx& g = *c->gen;
        const GenLayout& GL = g.L;
        g.rows_max = (std::max<int64_t>(c->MB, c->N) + 127) / 128 * 128;
        const size_t R = (size_t)g.rows_max;
        g.bf16 = cfg->compute_dtype == PPO_DTYPE_BF16;
        if (g.bf16) {
            // every bf16 buffer: 128 extra rows (the unguarded staging prefetches up to three chunks past the last one it uses), pitches padded
            // to 128 columns, zero-filled once -- nothing ever writes the padding
            g.ld_in0 = (GL.obs + 127) / 128 * 128;
            g.ld_h = (GL.hidden + 127) / 128 * 128;
            const size_t RB = R + 128;
            CK(dalloc(c, &g.xin_bf, RB * g.ld_in0));
            if (gen_rows_packable(GL)) CK(dalloc(c, &g.row_rec, (size_t)B * 8));
            CK(dalloc(c, &g.obs_bf, ((size_t)B + 128) * g.ld_in0));   // the rollout's observations as bf16, once per update (gen_fwd_bwd): 201 MB at 2048 x 128 x 384
            for (int net = 0; net < 2; net++)
                for (int l = 0; l < GL.n_hidden; l++) CK(dalloc(c, &g.acts_bf[net][l], RB * g.ld_h));
            for (int i = 0; i < 2; i++) {
                CK(dalloc(c, &g.tmp_bf[i], RB * g.ld_h));
                CK(dalloc(c, &g.dz_bf[0][i], RB * g.ld_h));
                CK(dalloc(c, &g.dz_bf[1][i], RB * g.ld_h));
                CK(dalloc(c, &g.dout_bf[i], RB * 128));
            }
            g.cs_layer_stride = (int64_t)(R / 64 + 2) * g.ld_h;   // one row of column sums per 64-row tile at most (kernels_generic_bwd.hip: a row range is >= one tile)
            CK(dalloc(c, &g.cs_part[0], (size_t)GL.n_layers * g.cs_layer_stride));
            CK(dalloc(c, &g.cs_part[1], (size_t)GL.n_layers * g.cs_layer_stride));
            CK(dalloc(c, &g.head_db_part, (size_t)GEN_LOSS_BLOCKS * (GL.act + 1)));
            {   // one pair of doubles per slab-sum workgroup (256 gradient elements: kernels_generic.hip SLAB_EPB) of the largest layer, per layer and net
                int64_t most = 0;
                for (int net = 0; net < 2; net++)
                    for (int l = 0; l < GL.n_layers; l++) most = std::max<int64_t>(most, (int64_t)GL.out_dim[net][l] * GL.in_dim[l] + GL.out_dim[net][l]);
                g.sq_cap = (int)((most + 255) / 256);
                CK(dalloc(c, &g.sq_part, (size_t)2 * GL.n_layers * g.sq_cap * 2));
            }
        } else {
            for (int net = 0; net < 2; net++)
                for (int l = 0; l < GL.n_hidden; l++) CK(dalloc(c, &g.acts[net][l], R * GL.hidden));
            for (int i = 0; i < 2; i++) CK(dalloc(c, &g.dz[i], R * GL.hidden));
            CK(dalloc(c, &g.xin, R * GL.obs));
            CK(dalloc(c, &g.dlogits, R * GL.act));
            CK(dalloc(c, &g.dval, R));
        }
        CK(dalloc(c, &g.logits, R * GL.act));
        CK(dalloc(c, &g.val, R));
        for (int i = 0; i < 4; i++) CK(dalloc(c, &g.row_f[i], R));
        CK(dalloc(c, &g.row_f[4], R + 2));
        CK(dalloc(c, &g.row_act, R * gen_action_words(GL)));
        CK(dalloc(c, &g.row_mask, R * GL.act));

        CK(dalloc(c, &g.loss_part, (size_t)GEN_LOSS_BLOCKS * 8));
        {
            int64_t mx = 0;
            for (int l = 0; l < GL.n_layers; l++) mx = std::max<int64_t>(mx, (int64_t)std::max(GL.out_dim[0][l], GL.out_dim[1][l]) * (GL.in_dim[l] + 1));
            g.wslab_stride = (mx + 3) & ~3ll;
            // bf16 storage: a block of slabs per layer (a net's slab sums are ONE launch behind its backward pass: 10 launches less per minibatch step);
            // 5 layers x 129 slabs x 386 KB x 2 nets = 0.5 GB of 288
            g.wslab_layer_stride = (int64_t)(GEN_SPLIT_MFMA + 1) * g.wslab_stride;
            CK(dalloc(c, &g.wslab, (size_t)(g.bf16 ? GL.n_layers : 1) * g.wslab_layer_stride));
            if (g.bf16) {
                CK(dalloc(c, &g.wslab1, (size_t)GL.n_layers * g.wslab_layer_stride));
                CK(hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking));
                CK(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
                CK(hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming));
                CK(hipEventCreateWithFlags(&c->ev_gather, hipEventDisableTiming));
            }
            CK(dalloc(c, &g.db_part, (size_t)GEN_DB_CHUNKS * std::max(GL.hidden, GL.act)));
        }
        {   // bf16 planes of every layer's weights, padded to tile multiples (kernels_gemm.hip: PlaneStage)
            int64_t off = 0;
            for (int net = 0; net < 2; net++)
                for (int l = 0; l < GL.n_layers; l++) {
                    g.wp_npad[net][l] = (GL.out_dim[net][l] + 127) / 128 * 128;
                    g.wp_kpad[l] = (GL.in_dim[l] + 127) / 128 * 128;   // the tiled kernel's chunking; the fused kernels walk it in passes of 8 k steps
                    g.wp_off[net][l] = off;
                    off += 3ll * g.wp_npad[net][l] * g.wp_kpad[l];
                }
            CK(dalloc(c, &g.wplanes, (size_t)off + 128 * 256));   // + slack for the staging's prefetch past the last chunk
            if (cfg->compute_dtype == PPO_DTYPE_BF16) CK(dalloc(c, &g.wfrags, (size_t)off + 128 * 256));
            g.planes_dirty = true;
        }
        CK(dalloc(c, &g.act64, N * GL.n_heads));
        CK(dalloc(c, &g.step_lp, N));
        CK(dalloc(c, &g.step_en, N));
        if (GL.gauss) {
            CK(dalloc(c, &g.actf, N * GL.gauss));
            CK(dalloc(c, &g.ls_part, (size_t)GEN_LOSS_BLOCKS * GL.gauss));
        }
        if (gauss_fused || cat_fused) {
            c->gauss_fused = gauss_fused;
            c->cat_fused = cat_fused;
            CK(dalloc(c, &c->gf_slab, (size_t)2 * GAUSS_FUSED_MAX_BLOCKS * gauss_fused_slab_stride(GL)));
        }
        CK(dalloc(c, &c->cur_mask, N * GL.act));
        if (env && (cfg->kernel_flags & PPO_KERNEL_ENV_CUT_STATE)) CK(dalloc(c, &c->cut_state, (size_t)(env->state + 1) * TN));
        if (env && (cfg->kernel_flags & PPO_KERNEL_ENV_REWARD_NORM)) CK(dalloc(c, &c->rn_ws, rewnorm_rollout_workspace(cfg->num_envs, cfg->num_steps)));
        if (env_generic) {   // CartPole::getActionMask / MountainCar::getActionMask are all ones (MountainCar.cpp:69-77): the mask of every step under PPO_DIST_MASKED
            c->env_generic = true;
            CK(hipMemset(c->cur_mask, 1, N * GL.act));
        }
        // the zero-fills above ran on the null stream, which a non-blocking stream does not wait for: drain them before the first write
        CK(hipDeviceSynchronize());
        CK(gen_fill(g.row_f[4] + 2, (int64_t)R, 1.0f, c->stream));   // the ones vector of the bias-gradient gemv
        // arithmetic of the layer products (kernels_gemm.hip): fp32 carried as three bf16 terms, or plain bf16 operands (configs[4])
        g.gemm_prec = cfg->compute_dtype == PPO_DTYPE_BF16 ? PPO_MM_BF16 : PPO_MM_F32X3;
    }
#undef CK
    // every env can reset at most once per step: steps per env over the whole run bounds the shared reset stream
    const int64_t steps_per_env = cfg->total_timesteps > 0 ? cfg->total_timesteps / std::max<int64_t>(c->cfg.global_num_envs, 1) : 0;
    ppo_status st = ensure_reset_table(c, std::max<int64_t>(steps_per_env + cfg->num_steps + 4, 4096));
    if (st != PPO_OK) { g_create_error = c->err; ppo_ctx_destroy(c); return st; }
    // the zero-fills of the allocations ran on the null stream, which the context's non-blocking stream does not wait for
    if (hipDeviceSynchronize() != hipSuccess) { fail(nullptr, PPO_ERR_HIP, "hipDeviceSynchronize failed at the end of ppo_ctx_create"); ppo_ctx_destroy(c); return PPO_ERR_HIP; }
    *out = c;
    return PPO_OK;
}

extern "C" ppo_status ppo_sync(ppo_ctx* c) {
    NEED(c, c != nullptr, "null ctx");
    DeviceGuard dev_guard(c);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return comm_health(c);
}
extern "C" void* ppo_stream(ppo_ctx* c) { return c ? c->stream : nullptr; }
extern "C" ppo_status ppo_get_config(const ppo_ctx* c, ppo_config* out) {
    if (!c || !out) return PPO_ERR_INVALID;
    *out = c->cfg;
    return PPO_OK;
}
extern "C" ppo_status ppo_buffer(ppo_ctx* c, int32_t which, void** dev_ptr, size_t* bytes) {
    NEED(c, c != nullptr, "null ctx");
    NEED(c, which >= 0 && which < PPO_BUF_COUNT_, "unknown buffer id");
    if (dev_ptr) *dev_ptr = c->buf[which];
    if (bytes) *bytes = c->buf_bytes[which];
    return PPO_OK;
}
extern "C" ppo_status ppo_device_alloc(ppo_ctx* c, size_t bytes, void** dev_ptr) {
    NEED(c, c && dev_ptr, "null argument");
    DeviceGuard dev_guard(c);
    HIPCHK(c, hipSetDevice(c->cfg.device));
    HIPCHK(c, hipMalloc(dev_ptr, std::max<size_t>(bytes, 16)));
    return PPO_OK;
}
extern "C" ppo_status ppo_device_free(ppo_ctx* c, void* dev_ptr) {
    NEED(c, c != nullptr, "null ctx");
    DeviceGuard dev_guard(c);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipFree(dev_ptr));
    return PPO_OK;
}
extern "C" ppo_status ppo_memcpy_h2d(ppo_ctx* c, void* dst_dev, const void* src_h, size_t bytes) {
    NEED(c, c != nullptr, "null ctx");
    DeviceGuard dev_guard(c);
    HIPCHK(c, hipMemcpyAsync(dst_dev, src_h, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->gen) { c->gen->planes_dirty = true; c->gen_opt_fused_ok = false; }   // the copy may have landed in the parameters (re-split the weights before their next use) or in the gradient
    c->wrange_dirty = true;                    // ... and their fp16-range maxima are recomputed before the next matrix-core launch
    return PPO_OK;
}
extern "C" ppo_status ppo_memcpy_d2h(ppo_ctx* c, void* dst_h, const void* src_dev, size_t bytes) {
    NEED(c, c != nullptr, "null ctx");
    DeviceGuard dev_guard(c);
    HIPCHK(c, hipMemcpyAsync(dst_h, src_dev, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PPO_OK;
}

// ---------------------------------------------------------------------------------------------------------
// Agent
// ---------------------------------------------------------------------------------------------------------
extern "C" int64_t ppo_param_count(const ppo_ctx* c) { return c ? c->L.P : -1; }

extern "C" ppo_status ppo_param_shapes(const ppo_ctx* c, int64_t* shapes_h, int32_t* n_tensors) {
    if (!c) return PPO_ERR_INVALID;
    if (n_tensors) *n_tensors = c->L.n_tensors;
    if (shapes_h && c->gen) {
        const GenLayout& GL = c->gen->L;
        int k = 0;
        for (int net = 0; net < 2; net++)
            for (int l = 0; l < GL.n_layers; l++) {
                shapes_h[k++] = GL.out_dim[net][l]; shapes_h[k++] = GL.in_dim[l];
                shapes_h[k++] = GL.out_dim[net][l]; shapes_h[k++] = 1;
            }
        if (GL.gauss) { shapes_h[k++] = GL.gauss; shapes_h[k++] = 1; }   // log_std [D], the last tensor
        return PPO_OK;
    }
    if (shapes_h) {
        int k = 0;
        for (int net = 0; net < 2; net++) {
            const int out3 = net == 0 ? 1 : c->A;
            const int64_t dims[6][2] = { { PPO_HIDDEN, c->O }, { PPO_HIDDEN, 1 }, { PPO_HIDDEN, PPO_HIDDEN }, { PPO_HIDDEN, 1 }, { out3, PPO_HIDDEN }, { out3, 1 } };
            for (auto& d : dims) { shapes_h[k++] = d[0]; shapes_h[k++] = d[1]; }
        }
    }
    return PPO_OK;
}

extern "C" ppo_status ppo_params_set_h(ppo_ctx* c, const float* params_h, int64_t count) {
    NEED(c, c && params_h, "null argument");
    NEED(c, count == c->L.P, "parameter count mismatch");
    return ppo_memcpy_h2d(c, c->buf[PPO_BUF_PARAMS], params_h, (size_t)count * sizeof(float));
}
extern "C" ppo_status ppo_params_get_h(ppo_ctx* c, float* params_h, int64_t count) {
    NEED(c, c && params_h, "null argument");
    NEED(c, count == c->L.P, "parameter count mismatch");
    return ppo_memcpy_d2h(c, params_h, c->buf[PPO_BUF_PARAMS], (size_t)count * sizeof(float));
}
static ppo_status es_resolve(ppo_ctx* c);
extern "C" ppo_status ppo_optimizer_set_h(ppo_ctx* c, const float* m_h, const float* v_h, int64_t count, int64_t step) {
    NEED(c, c && m_h && v_h, "null argument");
    NEED(c, count == c->L.P, "parameter count mismatch");
    ppo_status s = ppo_memcpy_h2d(c, c->buf[PPO_BUF_EXP_AVG], m_h, (size_t)count * sizeof(float));
    if (s != PPO_OK) return s;
    s = ppo_memcpy_h2d(c, c->buf[PPO_BUF_EXP_AVG_SQ], v_h, (size_t)count * sizeof(float));
    if (s != PPO_OK) return s;
    s = es_resolve(c);
    if (s != PPO_OK) return s;
    c->opt_step = step;
    return s;
}
extern "C" ppo_status ppo_optimizer_get_h(ppo_ctx* c, float* m_h, float* v_h, int64_t count, int64_t* step) {
    NEED(c, c != nullptr, "null ctx");
    NEED(c, count == c->L.P, "parameter count mismatch");
    ppo_status s = PPO_OK;
    if (m_h) s = ppo_memcpy_d2h(c, m_h, c->buf[PPO_BUF_EXP_AVG], (size_t)count * sizeof(float));
    if (s == PPO_OK && v_h) s = ppo_memcpy_d2h(c, v_h, c->buf[PPO_BUF_EXP_AVG_SQ], (size_t)count * sizeof(float));
    if (s == PPO_OK && step) {
        s = es_resolve(c);   // applied steps: an update that stopped at its target KL applied fewer than it enqueued
        *step = c->opt_step;
    }
    return s;
}

// Agent::ppoLayerInit (Agent.cpp:91-99): torch::nn::init::orthogonal_(W, gain) = gain * Q of a Gaussian matrix (QR with the
// sign of diag(R) folded in), constant_(bias, 0).  LibTorch draws the Gaussian from its global mt19937 and calls LAPACK;
// here: Box-Muller on Philox(seed; tensor, element) and Householder QR in binary64.  Distributionally equivalent, not bit-equal.
static void orthogonal_fill(float* W, int rows, int cols, double gain, int64_t seed, int tensor_id) {
    const bool transpose = rows < cols;
    const int m = transpose ? cols : rows, n = transpose ? rows : cols;  // m >= n
    std::vector<double> Aq((size_t)m * n);
    auto philox_host = [&](uint32_t c0, uint32_t c1, uint32_t out[4]) {
        uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)((uint64_t)seed >> 32), c2 = (uint32_t)tensor_id, c3 = 3u;
        for (int r = 0; r < 10; r++) {
            const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
            const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
            c0 = n0; c1 = n1; c2 = n2; c3 = n3;
            k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
        }
        out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
    };
    for (size_t i = 0; i < Aq.size(); i += 2) {
        uint32_t w[4];
        philox_host((uint32_t)i, (uint32_t)(i >> 32), w);
        const double u1 = ((double)w[0] + 1.0) / 4294967296.0, u2 = (double)w[1] / 4294967296.0;
        const double r = std::sqrt(-2.0 * std::log(u1));
        Aq[i] = r * std::cos(2.0 * M_PI * u2);
        if (i + 1 < Aq.size()) Aq[i + 1] = r * std::sin(2.0 * M_PI * u2);
    }
    // Householder QR of Aq (m x n, row-major); accumulate Q (m x n) explicitly.
    std::vector<double> R = Aq, Q((size_t)m * n, 0.0), v((size_t)m);
    std::vector<std::vector<double>> vs;
    for (int k = 0; k < n; k++) {
        double norm = 0.0;
        for (int i = k; i < m; i++) norm += R[(size_t)i * n + k] * R[(size_t)i * n + k];
        norm = std::sqrt(norm);
        std::fill(v.begin(), v.end(), 0.0);
        const double alpha = R[(size_t)k * n + k] >= 0 ? -norm : norm;
        for (int i = k; i < m; i++) v[i] = R[(size_t)i * n + k];
        v[k] -= alpha;
        double vn = 0.0;
        for (int i = k; i < m; i++) vn += v[i] * v[i];
        if (vn > 0) {
            for (int j = k; j < n; j++) {
                double dot = 0.0;
                for (int i = k; i < m; i++) dot += v[i] * R[(size_t)i * n + j];
                const double f = 2.0 * dot / vn;
                for (int i = k; i < m; i++) R[(size_t)i * n + j] -= f * v[i];
            }
        }
        vs.push_back(v);
    }
    for (int j = 0; j < n; j++) Q[(size_t)j * n + j] = 1.0;
    for (int k = n - 1; k >= 0; k--) {
        const std::vector<double>& vk = vs[k];
        double vn = 0.0;
        for (int i = k; i < m; i++) vn += vk[i] * vk[i];
        if (vn <= 0) continue;
        for (int j = 0; j < n; j++) {
            double dot = 0.0;
            for (int i = k; i < m; i++) dot += vk[i] * Q[(size_t)i * n + j];
            const double f = 2.0 * dot / vn;
            for (int i = k; i < m; i++) Q[(size_t)i * n + j] -= f * vk[i];
        }
    }
    for (int j = 0; j < n; j++) {
        const double sgn = R[(size_t)j * n + j] < 0 ? -1.0 : 1.0;  // q *= sign(diag(r))
        for (int i = 0; i < m; i++) Q[(size_t)i * n + j] *= sgn;
    }
    for (int r = 0; r < rows; r++)
        for (int cc = 0; cc < cols; cc++) W[(size_t)r * cols + cc] = (float)(gain * (transpose ? Q[(size_t)cc * n + r] : Q[(size_t)r * n + cc]));
}

extern "C" ppo_status ppo_params_init_orthogonal(ppo_ctx* c, int64_t seed) {
    NEED(c, c != nullptr, "null ctx");
    DeviceGuard dev_guard(c);
    std::vector<float> p((size_t)c->L.P, 0.0f);
    if (c->gen) {   // Agent.cpp:25-59 generalised: sqrt(2) on hidden layers, 1.0 on the value head, 0.01 on the policy head
        const GenLayout& GL = c->gen->L;
        for (int net = 0; net < 2; net++)
            for (int l = 0; l < GL.n_layers; l++) {
                const double gain = l < GL.n_hidden ? std::sqrt(2.0) : (net == 0 ? 1.0 : 0.01);
                orthogonal_fill(p.data() + GL.w_off[net][l], GL.out_dim[net][l], GL.in_dim[l], gain, seed, net * GEN_MAX_LAYERS + l);
            }
        // Gaussian policies: log_std = 0 (sigma = 1), like every bias
        return ppo_params_set_h(c, p.data(), c->L.P);
    }
    for (int net = 0; net < 2; net++) {
        const int out3 = net == 0 ? 1 : c->A;
        orthogonal_fill(p.data() + c->L.w1[net], PPO_HIDDEN, c->O, std::sqrt(2.0), seed, net * 3 + 0);
        orthogonal_fill(p.data() + c->L.w2[net], PPO_HIDDEN, PPO_HIDDEN, std::sqrt(2.0), seed, net * 3 + 1);
        orthogonal_fill(p.data() + c->L.w3[net], out3, PPO_HIDDEN, net == 0 ? 1.0 : 0.01, seed, net * 3 + 2);  // Agent.cpp:28,37
    }
    return ppo_params_set_h(c, p.data(), c->L.P);
}

// PPO_KERNEL_ENV_GENERIC with bf16 storage on MountainCar: generic_forward_kernel stages f32 rows as 16-byte pieces (obs_size % 4 == 0), which an observation
// of 2 is not.  Rounded to bf16 into g.xin_bf first (gen_forward's own first launch), the rows go through the fused layers the rollout kernel runs, so
// ppo_policy_act and ppo_get_value give a row the one-launch rollout's logits and value, bit for bit, as they do on CartPole.
static inline bool env_generic_via_bf16(const ppo_ctx* c) { return c->env_generic && gen_fused_ok(*c->gen) && !gen_fused_forward_ok(*c->gen); }
static ppo_status gen_fused_rows_via_bf16(ppo_ctx* c, int net, const float* obs, int64_t rows, float* out) {
    GenericCtx& g = *c->gen;
    NEED(c, rows <= g.rows_max, "more rows than the workspace holds");
    HIPCHK(c, launch_to_bf16_pad(obs, rows, g.L.obs, g.xin_bf, g.ld_in0, c->stream));
    HIPCHK(c, gen_fused_forward(g, B_<float>(c, PPO_BUF_PARAMS), net, nullptr, g.xin_bf, g.ld_in0, rows, false, out, c->stream));
    return PPO_OK;
}

// ---- generic networks (generic.hpp): critic / actor over n rows, chunked to the workspace size ----
static ppo_status gen_values(ppo_ctx* c, const float* obs, int64_t n, float* value) {
    GenericCtx& g = *c->gen;
    if (env_generic_via_bf16(c)) {
        for (int64_t off = 0; off < n; off += g.rows_max) {
            const ppo_status s = gen_fused_rows_via_bf16(c, 0, obs + off * g.L.obs, std::min<int64_t>(g.rows_max, n - off), value + off);
            if (s != PPO_OK) return s;
        }
        return PPO_OK;
    }
    if (c->gauss_fused || c->cat_fused) {   // PPO_KERNEL_GAUSS_FUSED / PPO_KERNEL_CAT_FUSED: the critic over all n rows in one launch (the kernel is distribution-free)
        NEED(c, n < (1ll << 31), "more than 2^31 rows");
        if (n > 0) c->gf_launches[1] += 1;
        HIPCHK(c, gauss_fused_values(g.L, B_<float>(c, PPO_BUF_PARAMS), obs, n, value, c->stream));
        return PPO_OK;
    }
    if (gen_fused_forward_ok(g) && n <= GEN_FUSED_MAX_ROWS) {   // bf16 storage, small batch: the whole critic in one launch
        HIPCHK(c, gen_fused_forward(g, B_<float>(c, PPO_BUF_PARAMS), 0, obs, nullptr, 0, n, false, value, c->stream));
        return PPO_OK;
    }
    for (int64_t off = 0; off < n; off += g.rows_max) {
        const int64_t rows = std::min<int64_t>(g.rows_max, n - off);
        HIPCHK(c, gen_forward(g, B_<float>(c, PPO_BUF_PARAMS), 0, obs + off * g.L.obs, rows, nullptr, g.dz[0], g.dz[1], value + off, c->stream));
    }
    return PPO_OK;
}
// row0 / key_rows (env groups: the n rows are rows row0 .. of a batch of key_rows): the sampler's row origin, and the row count that picks between the fused
// forward and the per-layer products -- the one launch choice here that follows the row count and changes bits -- so that a group's rows get what the
// whole batch would.  It only matters for N > GEN_FUSED_MAX_ROWS = 2^20 (rows_max >= N: the ungrouped call is one chunk of N rows).  THAT switch stays
// untested: a context of more than 2^20 envs needs workspaces of several gigabytes, too much for a suite that shares its machines.
// gen_forward's own choices by row count are left alone: launch_prec takes the double-buffered variant for M <= 8192 (three-term product), and both variants
// walk the k chunks in ascending order with the same MFMAs per chunk, so a row's bits do not depend on the variant; its 32 x 128 tile for M <= 32 is never
// taken here (gen_forward always passes weight planes).  Two tests hold that: tests/test_gpu_matmul.py::test_matmul_main_loops_agree_bit_for_bit (8320 rows
// in one product against the same rows as 8192 + 128, every operand orientation, with and without the bias + tanh epilogue) and
// tests/test_gpu_host_env_groups.py::test_grouped_generic_f32_across_the_gemm_threshold (8320 envs ungrouped against two groups of 4160, weight planes,
// every buffer and the parameters after the update); the same file covers groups of 7 .. 32 rows in batches of 50 / 64.
// PPO_KERNEL_CAT_FUSED: forward, heads and -- when `stores` is given -- the step's rollout stores in ONE launch over the n rows, whose sampler origin is
// env_offset + row0; returns true in *stored then (the caller skips gen_store_step)
static ppo_status gen_policy(ppo_ctx* c, const float* obs, const uint8_t* mask, const int64_t* forced, int64_t n, int64_t step_index, int64_t* action,
                             float* logprob, float* entropy, bool greedy = false, int64_t row0 = 0, int64_t key_rows = 0, const CatStepStores* stores = nullptr,
                             bool* stored = nullptr) {
    GenericCtx& g = *c->gen;
    if (stored) *stored = false;
    if (c->cat_fused) {
        NEED(c, n < (1ll << 31), "more than 2^31 rows");
        if (n > 0) c->gf_launches[0] += 1;
        HIPCHK(c, cat_fused_act(g.L, c->cfg.dist_kind, B_<float>(c, PPO_BUF_PARAMS), obs, mask, greedy ? nullptr : forced, n, c->cfg.seed, c->cfg.env_offset + row0,
                                step_index, greedy, action, logprob, entropy, stores, c->stream));
        if (stored) *stored = stores != nullptr;
        return PPO_OK;
    }
    for (int64_t off = 0; off < n; off += g.rows_max) {
        const int64_t rows = std::min<int64_t>(g.rows_max, n - off);
        if (env_generic_via_bf16(c)) {
            const ppo_status s = gen_fused_rows_via_bf16(c, 1, obs + off * g.L.obs, rows, g.logits);
            if (s != PPO_OK) return s;
        } else if (gen_fused_forward_ok(g) && (key_rows > 0 ? std::min<int64_t>(g.rows_max, key_rows) : rows) <= GEN_FUSED_MAX_ROWS) HIPCHK(c, gen_fused_forward(g, B_<float>(c, PPO_BUF_PARAMS), 1, obs + off * g.L.obs, nullptr, 0, rows, false, g.logits, c->stream));
        else HIPCHK(c, gen_forward(g, B_<float>(c, PPO_BUF_PARAMS), 1, obs + off * g.L.obs, rows, nullptr, g.dz[0], g.dz[1], g.logits, c->stream));
        HIPCHK(c, gen_heads(g.L, c->cfg.dist_kind, g.logits, mask ? mask + off * g.L.act : nullptr, forced ? forced + off * g.L.n_heads : nullptr, rows,
                            c->cfg.seed, c->cfg.env_offset + row0 + off, step_index, action ? action + off * g.L.n_heads : nullptr,
                            logprob ? logprob + off : nullptr, entropy ? entropy + off : nullptr, c->stream, greedy));
    }
    return PPO_OK;
}

// gen_policy for a Gaussian context: the actor's forward gives the mean, gauss_heads_kernel the action (f32 [n, D]), its log-prob and the entropy.
// PPO_KERNEL_GAUSS_FUSED: all of it, and the step's rollout stores when `stores` is given, in ONE launch; returns true in *stored then (the caller skips
// gen_gauss_store_step)
static ppo_status gen_policy_gauss(ppo_ctx* c, const float* obs, const float* forced, int64_t n, int64_t step_index, float* action, float* logprob, float* entropy,
                                   bool greedy = false, const GaussStepStores* stores = nullptr, bool* stored = nullptr) {
    GenericCtx& g = *c->gen;
    const int D = g.L.gauss;
    const float* params = B_<float>(c, PPO_BUF_PARAMS);
    if (stored) *stored = false;
    if (c->gauss_fused) {
        NEED(c, n < (1ll << 31), "more than 2^31 rows");
        if (n > 0) c->gf_launches[0] += 1;
        HIPCHK(c, gauss_fused_act(g.L, params, obs, forced, n, c->cfg.seed, c->cfg.env_offset, step_index, greedy, action, logprob, entropy, stores, c->stream));
        if (stored) *stored = stores != nullptr;
        return PPO_OK;
    }
    for (int64_t off = 0; off < n; off += g.rows_max) {
        const int64_t rows = std::min<int64_t>(g.rows_max, n - off);
        HIPCHK(c, gen_forward(g, params, 1, obs + off * g.L.obs, rows, nullptr, g.dz[0], g.dz[1], g.logits, c->stream));
        HIPCHK(c, gen_gauss_heads(D, g.logits, params + g.L.logstd_off, forced ? forced + off * D : nullptr, rows, c->cfg.seed, c->cfg.env_offset + off, step_index,
                                  action ? action + off * D : nullptr, logprob ? logprob + off : nullptr, entropy ? entropy + off : nullptr, c->stream, greedy));
    }
    return PPO_OK;
}
static inline bool is_gauss(const ppo_ctx* c) { return c->cfg.dist_kind == PPO_DIST_GAUSSIAN; }
// the integer-action entry points on a Gaussian context, and the _f32 ones on a categorical context
static ppo_status wrong_action_type(ppo_ctx* c, const char* what, const char* other) {
    return is_gauss(c) ? fail(c, PPO_ERR_UNSUPPORTED, "%s: this context's policy is PPO_DIST_GAUSSIAN and its actions are f32 [n, D]; call %s", what, other)
                       : fail(c, PPO_ERR_UNSUPPORTED, "%s: this context's policy is categorical and its actions are i64 [n, H]; call %s", what, other);
}

extern "C" ppo_status ppo_get_value(ppo_ctx* c, const float* obs, int64_t n, float* value) {
    NEED(c, c && obs && value, "null argument");
    DeviceGuard dev_guard(c);
    if (c->gen) return gen_values(c, obs, n, value);
    HIPCHK(c, launch_policy_act(B_<float>(c, PPO_BUF_PARAMS), c->L, c->cfg.dist_kind, obs, nullptr, nullptr, n, c->cfg.seed, c->cfg.env_offset, 0,
                                nullptr, nullptr, nullptr, value, true, c->stream));
    return PPO_OK;
}

static ppo_status refresh_weight_range(ppo_ctx* c);          // (the fp16 range of the matrix-core kernels' operands: defined with ppo_rollout below)
static inline void wr_snapshot(ppo_ctx* c);
static inline bool weights_fit_rollout16(const ppo_ctx* c);

// ppo_policy_act and ppo_policy_act_greedy: one body.  greedy: the heads' modes instead of draws (no random number, forced_action unused).
static ppo_status policy_act_common(ppo_ctx* c, const float* obs, const uint8_t* mask, const int64_t* forced_action, int64_t n, int64_t step_index,
                                    int64_t* action, float* logprob, float* entropy, float* value, bool greedy) {
    if (c->gen) {
        ppo_status s = gen_policy(c, obs, mask, forced_action, n, step_index, action, logprob, entropy, greedy);
        if (s == PPO_OK && value) s = gen_values(c, obs, n, value);
        return s;
    }
    // The stand-alone policy runs the arithmetic of the kernel this context's ROLLOUT would run now (round 6): rollout16_kernel's two-term fp16 products
    // on the matrix cores by default, the vector ALU's fp32 multiply-adds under PPO_KERNEL_ROLLOUT_VECTOR or while the output layer's weights do not fit
    // (the same range snapshot, the same decision as ppo_rollout) -- so a caller comparing the two on the same observations sees the same bits.
    bool as16 = !c->rollout_vector && policy_act16_serves(c->L);
    if (as16) {
        const ppo_status rs = refresh_weight_range(c);
        if (rs != PPO_OK) return rs;
        wr_snapshot(c);
        if (!weights_fit_rollout16(c)) { as16 = false; c->vector_fallback_launches += 1; }
    }
    HIPCHK(c, launch_policy_act(B_<float>(c, PPO_BUF_PARAMS), c->L, c->cfg.dist_kind, obs, mask, forced_action, n, c->cfg.seed, c->cfg.env_offset,
                                step_index, action, logprob, entropy, value, false, c->stream, as16, c->error_flag, greedy));
    return PPO_OK;
}

extern "C" ppo_status ppo_policy_act(ppo_ctx* c, const float* obs, const uint8_t* mask, const int64_t* forced_action, int64_t n,
                                     int64_t step_index, int64_t* action, float* logprob, float* entropy, float* value) {
    NEED(c, c && obs, "null argument");
    if (is_gauss(c)) return wrong_action_type(c, "ppo_policy_act", "ppo_policy_act_f32");
    DeviceGuard dev_guard(c);
    NEED(c, forced_action || action, "sampling needs an action output");
    return policy_act_common(c, obs, mask, forced_action, n, step_index, action, logprob, entropy, value, false);
}

extern "C" ppo_status ppo_policy_act_f32(ppo_ctx* c, const float* obs, const float* forced_action, int64_t n, int64_t step_index, int32_t greedy,
                                         float* action, float* logprob, float* entropy, float* value) {
    NEED(c, c && obs, "null argument");
    if (!is_gauss(c)) return wrong_action_type(c, "ppo_policy_act_f32", greedy ? "ppo_policy_act_greedy" : "ppo_policy_act");
    NEED(c, n >= 0, "n < 0");
    NEED(c, forced_action || action, "sampling needs an action output");
    DeviceGuard dev_guard(c);
    ppo_status s = gen_policy_gauss(c, obs, greedy ? nullptr : forced_action, n, step_index, action, logprob, entropy, greedy != 0);
    if (s == PPO_OK && value) s = gen_values(c, obs, n, value);
    return s;
}

extern "C" ppo_status ppo_policy_act_greedy(ppo_ctx* c, const float* obs, const uint8_t* mask, int64_t n, int64_t* action, float* logprob, float* entropy,
                                            float* value) {
    NEED(c, c && obs, "null argument");
    if (is_gauss(c)) return wrong_action_type(c, "ppo_policy_act_greedy", "ppo_policy_act_f32 with greedy = 1");
    DeviceGuard dev_guard(c);
    NEED(c, action != nullptr, "ppo_policy_act_greedy needs an action output");
    NEED(c, n >= 0, "n < 0");
    return policy_act_common(c, obs, mask, nullptr, n, 0, action, logprob, entropy, value, true);
}

extern "C" ppo_status ppo_gauss_fused_launches(ppo_ctx* c, int64_t* act, int64_t* value, int64_t* update) {
    NEED(c, c != nullptr, "null ctx");
    if (act) *act = c->gf_launches[0];
    if (value) *value = c->gf_launches[1];
    if (update) *update = c->gf_launches[2];
    return PPO_OK;
}

extern "C" ppo_status ppo_categorical(int32_t dist_kind, const float* logits, const uint8_t* mask, const int64_t* value, int64_t n, int32_t A,
                                      float* m_logits, float* m_probs, float* log_prob, float* entropy, int64_t* mode, void* stream) {
    if (!logits || n < 0) return PPO_ERR_INVALID;
    return launch_categorical(dist_kind, logits, mask, value, n, A, m_logits, m_probs, log_prob, entropy, mode, (hipStream_t)stream) == hipSuccess ? PPO_OK : PPO_ERR_HIP;
}

extern "C" ppo_status ppo_gaussian(const float* mean, const float* log_std, const float* value, int64_t n, int32_t D, int64_t seed, int64_t row_offset,
                                   int64_t step_index, float* sample, float* log_prob, float* entropy, void* stream) {
    if (!mean || !log_std || n < 0 || D < 1 || D > PPO_MAX_ACT) return PPO_ERR_INVALID;
    return gen_gauss_heads(D, mean, log_std, value, n, seed, row_offset, step_index, sample, log_prob, entropy, (hipStream_t)stream) == hipSuccess ? PPO_OK : PPO_ERR_HIP;
}

extern "C" ppo_status ppo_categorical_sample(const float* m_probs, int64_t n, int32_t A, int64_t seed, int64_t row_offset, int64_t step_index,
                                             int32_t head, int64_t* sample, void* stream) {
    if (!m_probs || !sample || n < 0) return PPO_ERR_INVALID;
    return launch_categorical_sample(m_probs, n, A, seed, row_offset, step_index, head, sample, (hipStream_t)stream) == hipSuccess ? PPO_OK : PPO_ERR_HIP;
}

// ---------------------------------------------------------------------------------------------------------
// Environments
// ---------------------------------------------------------------------------------------------------------
extern "C" ppo_status ppo_env_transition(int32_t env_kind, const float* state_in, const int64_t* action, int64_t n, float* next_state,
                                         float* reward, int32_t* terminated, void* stream) {
    if (!state_in || !action || !next_state || !reward || !terminated || n < 0) return PPO_ERR_INVALID;
    const FusedEnvInfo* env = fused_env_info(env_kind);
    if (env && env->family == FUSED_CAT)   // state [n, STATE]
        return launch_cat_env_transition(env_kind, state_in, action, n, next_state, reward, terminated, (hipStream_t)stream) == hipSuccess ? PPO_OK : PPO_ERR_HIP;
    return launch_env_transition(env_kind, state_in, action, n, next_state, reward, terminated, (hipStream_t)stream) == hipSuccess ? PPO_OK : PPO_ERR_HIP;
}

// PPO_ENV_HOST: the entry points that step the context's own device env refuse, and say what to call instead
static ppo_status host_env_refuses(ppo_ctx* c, const char* what) {
    return fail(c, PPO_ERR_UNSUPPORTED, "%s steps the context's device environment, but this context's environments are the caller's (PPO_ENV_HOST): drive "
                                        "them with ppo_host_env_reset, ppo_host_rollout_begin, ppo_host_act, ppo_host_observe and ppo_host_rollout_end", what);
}

// what the refusals of the caller-stepped entry points add on a PPO_KERNEL_ENV_GENERIC context: the flag changes the network's engine, not whose env it is
static inline const char* env_generic_note(const ppo_ctx* c) { return c->env_generic ? ", on the generic engine under PPO_KERNEL_ENV_GENERIC" : ""; }
// the device envs of the fused rollouts (gauss_fused.hpp: FusedEnvInfo), with real-valued and with integer actions
static inline bool is_gauss_env(const ppo_ctx* c) { return c->env && c->env->family == FUSED_GAUSS; }
static inline bool is_cat_env(const ppo_ctx* c) { return c->env && c->env->family == FUSED_CAT; }

extern "C" ppo_status ppo_env_transition_f32(int32_t env_kind, const float* state_in, const float* action, int64_t n, float* next_state, float* obs_out,
                                             float* reward, int32_t* terminated, void* stream) {
    if (!state_in || !action || !next_state || !reward || !terminated || n < 0) return PPO_ERR_INVALID;
    const FusedEnvInfo* env = fused_env_info(env_kind);
    if (!env || env->family != FUSED_GAUSS) return PPO_ERR_UNSUPPORTED;   // the envs with integer actions: ppo_env_transition
    return launch_gauss_env_transition(env_kind, state_in, action, n, next_state, obs_out, reward, terminated, (hipStream_t)stream) == hipSuccess ? PPO_OK : PPO_ERR_HIP;
}

extern "C" ppo_status ppo_env_reset(ppo_ctx* c) {
    NEED(c, c != nullptr, "null ctx");
    if (c->host_env) return host_env_refuses(c, "ppo_env_reset");
    DeviceGuard dev_guard(c);
    if (c->env) {
        HIPCHK(c, launch_fused_env_reset(c->cfg.env_kind, c->N, c->cfg.seed, c->cfg.env_offset, B_<float>(c, PPO_BUF_ENV_STATE), B_<int32_t>(c, PPO_BUF_EP_LEN), B_<float>(c, PPO_BUF_EP_REW),
                                        B_<int32_t>(c, PPO_BUF_RESET_COUNT), B_<float>(c, PPO_BUF_NEXT_OBS), B_<int32_t>(c, PPO_BUF_NEXT_DONE), c->stream));
        // reward normalisation (PPO_KERNEL_ENV_REWARD_NORM): every episode starts anew, so the return accumulators do; the statistics stay
        if (c->rn_ret) HIPCHK(c, hipMemsetAsync(c->rn_ret, 0, (size_t)c->N * sizeof(double), c->stream));
        return PPO_OK;
    }
    if (c->gen && !c->env_generic) {   // synthetic env: memoryless, the observation of global step `rollout_steps` (0 after creation)
        HIPCHK(c, hipMemsetAsync(c->buf[PPO_BUF_EP_LEN], 0, (size_t)c->N * sizeof(int32_t), c->stream));
        HIPCHK(c, hipMemsetAsync(c->buf[PPO_BUF_EP_REW], 0, (size_t)c->N * sizeof(float), c->stream));
        HIPCHK(c, hipMemsetAsync(c->buf[PPO_BUF_NEXT_DONE], 0, (size_t)c->N * sizeof(int32_t), c->stream));
        HIPCHK(c, gen_synthetic_step(c->gen->L, c->N, c->cfg.seed, c->cfg.env_offset, c->rollout_steps, c->cfg.max_episode_steps, nullptr, nullptr,
                                     B_<float>(c, PPO_BUF_NEXT_OBS), c->cur_mask, nullptr, nullptr, nullptr, nullptr, c->stream));
        return PPO_OK;
    }
    HIPCHK(c, launch_env_reset(c->cfg.env_kind, c->N, c->cfg.seed, c->cfg.env_offset, B_<float>(c, PPO_BUF_ENV_STATE), B_<int32_t>(c, PPO_BUF_EP_LEN),
                               B_<float>(c, PPO_BUF_EP_REW), B_<int32_t>(c, PPO_BUF_RESET_COUNT), c->reset_table, c->reset_cap,
                               B_<float>(c, PPO_BUF_NEXT_OBS), B_<int32_t>(c, PPO_BUF_NEXT_DONE), c->error_flag, c->stream));
    return PPO_OK;
}

extern "C" ppo_status ppo_env_step(ppo_ctx* c, const int64_t* action, float* obs, float* reward, int32_t* done) {
    NEED(c, c && action && obs && reward && done, "null argument");
    if (c->host_env) return host_env_refuses(c, "ppo_env_step");
    if (is_gauss_env(c)) return fail(c, PPO_ERR_UNSUPPORTED, "ppo_env_step: this context's env (%s) takes real-valued actions f32 [N, D]; call ppo_env_step_f32", c->env->name);
    DeviceGuard dev_guard(c);
    if (is_cat_env(c)) {
        HIPCHK(c, launch_cat_env_step(c->cfg.env_kind, c->N, c->cfg.max_episode_steps, c->cfg.seed, c->cfg.env_offset, B_<float>(c, PPO_BUF_ENV_STATE), B_<int32_t>(c, PPO_BUF_EP_LEN),
                                     B_<float>(c, PPO_BUF_EP_REW), B_<int32_t>(c, PPO_BUF_RESET_COUNT), action, obs, reward, done, c->stream));
        return PPO_OK;
    }
    if (c->gen && !c->env_generic) {   // synthetic env: one step at the context's global step counter (the action does not influence it)
        HIPCHK(c, gen_synthetic_step(c->gen->L, c->N, c->cfg.seed, c->cfg.env_offset, c->rollout_steps, c->cfg.max_episode_steps,
                                     B_<int32_t>(c, PPO_BUF_EP_LEN), B_<float>(c, PPO_BUF_EP_REW), obs, c->cur_mask, reward, done, nullptr, nullptr, c->stream));
        c->rollout_steps += 1;
        return PPO_OK;
    }
    HIPCHK(c, launch_env_step(c->cfg.env_kind, c->N, c->H, c->cfg.max_episode_steps, c->cfg.seed, c->cfg.env_offset, B_<float>(c, PPO_BUF_ENV_STATE),
                              B_<int32_t>(c, PPO_BUF_EP_LEN), B_<float>(c, PPO_BUF_EP_REW), B_<int32_t>(c, PPO_BUF_RESET_COUNT), c->reset_table,
                              c->reset_cap, action, obs, reward, done, c->error_flag, c->stream));
    return PPO_OK;
}

extern "C" ppo_status ppo_env_step_f32(ppo_ctx* c, const float* action, float* obs, float* reward, int32_t* done) {
    NEED(c, c && action && obs && reward && done, "null argument");
    if (c->host_env) return host_env_refuses(c, "ppo_env_step_f32");
    if (!is_gauss_env(c))
        return fail(c, PPO_ERR_UNSUPPORTED, "ppo_env_step_f32: this context's env (env_kind %d) takes integer actions i64 [N, H]; call ppo_env_step", c->cfg.env_kind);
    DeviceGuard dev_guard(c);
    HIPCHK(c, launch_gauss_env_step(c->cfg.env_kind, c->N, c->cfg.max_episode_steps, c->cfg.seed, c->cfg.env_offset, B_<float>(c, PPO_BUF_ENV_STATE), B_<int32_t>(c, PPO_BUF_EP_LEN),
                                   B_<float>(c, PPO_BUF_EP_REW), B_<int32_t>(c, PPO_BUF_RESET_COUNT), action, obs, reward, done, c->stream));
    return PPO_OK;
}

// the env state's width: a fused device env's row has it; the observation IS the state for CartPole and MountainCar
static inline int env_state_dim(const ppo_ctx* c) { return c->env ? c->env->state : c->O; }

extern "C" ppo_status ppo_env_set_state_h(ppo_ctx* c, const float* state_h, const int32_t* ep_len_h, const float* ep_rew_h, const int32_t* reset_count_h) {
    NEED(c, c != nullptr, "null ctx");
    DeviceGuard dev_guard(c);
    if (state_h && c->env && c->env->check.words) {   // the state's words are integers of known ranges: checked here, on the host array
        const FusedStateCheck& k = c->env->check;
        const int S = c->env->state;
        for (int64_t i = 0; i < (int64_t)c->N * S; i++) {
            const float v = state_h[i];
            const int w = (int)(i % S), hi = k.hi[w];
            const bool ok = v >= 0.0f && v <= (float)hi && v == (float)(int)v && (!k.word_ok || k.word_ok(w, (int)v));
            if (!ok && k.word_ok)   // a word with a condition beyond its bound: the message gives the ranges only
                return fail(c, PPO_ERR_INVALID, "ppo_env_set_state_h: state[%lld][%d] = %g is not an integer of its range (%s); nothing was changed",
                            (long long)(i / S), w, (double)v, k.words);
            if (!ok)
                return fail(c, PPO_ERR_INVALID, "ppo_env_set_state_h: state[%lld][%d] = %g is not an integer in 0..%d (%s); nothing was changed",
                            (long long)(i / S), w, (double)v, hi, k.words);
        }
    }
    if (state_h) {
        const int S = env_state_dim(c);
        ppo_status s = ppo_memcpy_h2d(c, c->scratch_obs, state_h, (size_t)c->N * S * sizeof(float));
        if (s != PPO_OK) return s;
        HIPCHK(c, launch_aos_to_soa(c->scratch_obs, B_<float>(c, PPO_BUF_ENV_STATE), c->N, S, true, c->stream));
        if (c->env && !c->env->obs_is_state) HIPCHK(c, launch_fused_env_obs(c->cfg.env_kind, c->N, B_<float>(c, PPO_BUF_ENV_STATE), B_<float>(c, PPO_BUF_NEXT_OBS), c->stream));
        else HIPCHK(c, hipMemcpyAsync(c->buf[PPO_BUF_NEXT_OBS], c->scratch_obs, (size_t)c->N * c->O * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    }
    ppo_status s = PPO_OK;
    if (ep_len_h) s = ppo_memcpy_h2d(c, c->buf[PPO_BUF_EP_LEN], ep_len_h, (size_t)c->N * sizeof(int32_t));
    if (s == PPO_OK && ep_rew_h) s = ppo_memcpy_h2d(c, c->buf[PPO_BUF_EP_REW], ep_rew_h, (size_t)c->N * sizeof(float));
    if (s == PPO_OK && reset_count_h) s = ppo_memcpy_h2d(c, c->buf[PPO_BUF_RESET_COUNT], reset_count_h, (size_t)c->N * sizeof(int32_t));
    if (s == PPO_OK) HIPCHK(c, hipStreamSynchronize(c->stream));
    return s;
}

extern "C" ppo_status ppo_env_get_state_h(ppo_ctx* c, float* state_h, int32_t* ep_len_h, float* ep_rew_h, int32_t* reset_count_h) {
    NEED(c, c != nullptr, "null ctx");
    DeviceGuard dev_guard(c);
    ppo_status s = PPO_OK;
    if (state_h) {
        const int S = env_state_dim(c);
        HIPCHK(c, launch_aos_to_soa(c->scratch_obs, B_<float>(c, PPO_BUF_ENV_STATE), c->N, S, false, c->stream));
        s = ppo_memcpy_d2h(c, state_h, c->scratch_obs, (size_t)c->N * S * sizeof(float));
    }
    if (s == PPO_OK && ep_len_h) s = ppo_memcpy_d2h(c, ep_len_h, c->buf[PPO_BUF_EP_LEN], (size_t)c->N * sizeof(int32_t));
    if (s == PPO_OK && ep_rew_h) s = ppo_memcpy_d2h(c, ep_rew_h, c->buf[PPO_BUF_EP_REW], (size_t)c->N * sizeof(float));
    if (s == PPO_OK && reset_count_h) s = ppo_memcpy_d2h(c, reset_count_h, c->buf[PPO_BUF_RESET_COUNT], (size_t)c->N * sizeof(int32_t));
    return s;
}

// ---------------------------------------------------------------------------------------------------------
// Rollout and advantages
// ---------------------------------------------------------------------------------------------------------
static ppo_status gen_rollout(ppo_ctx* c, const int64_t* forced);
static ppo_status consume_finished_episodes(ppo_ctx* c) {
    if (!c->fin_pending) return PPO_OK;
    // the rollout that left these episodes has already advanced rollout_steps by T
    HIPCHK(c, launch_episode_ring_update(B_<int32_t>(c, PPO_BUF_FIN_LEN), B_<float>(c, PPO_BUF_FIN_REW), c->T, c->N, c->row_counts, c->group_bits, c->ring,
                                         c->rollout_steps - c->T, c->cfg.global_num_envs, c->cfg.env_offset, c->stream));
    c->fin_pending = false;
    return PPO_OK;
}

// The matrix-core kernels of the reference's two shapes carry some operands as fp16 (kernels_rollout.hip: 2^8 W3; kernels_update_mfma.hip: c W2 and the
// products through its columns); the reference has no such limits.  A drop-in user never sees them: weight_range_kernel takes the maxima of |parameter| per
// class once per update on a stream of its own (sweep_weight_range below; ppo_internal.hpp has the cost bisect), the host reads the pinned mirror -- no
// synchronisation; it lags the device by the launches in flight, during which AdamW moves a weight by about lr per step, hence thresholds at HALF the
// kernels' limits -- and a launch whose weights are out of range takes the vector kernel (plain fp32, same function; counted in
// ppo_profile.vector_fallback_launches).  After the host wrote parameters the maxima are recomputed from scratch (one tiny launch + a synchronisation).
constexpr float WR_LIMIT_W3 = 128.0f;    // rollout16_kernel: |W3| < 255
constexpr float WR_LIMIT_W2 = 4.0f;      // update kernels: a column of c W2 with absolute sum ~2^10 overflows the fp16 terms of dz1: 64 x 4 x 2.885 = 739
constexpr float WR_LIMIT_REST = 8192.0f; // c W1, c b1, c b2: < 65 504 / 2.885
static inline void wr_snapshot(ppo_ctx* c) {
    for (int i = 0; i < 3; i++) {
        const uint32_t bits = __atomic_load_n(c->wr_host + i, __ATOMIC_RELAXED);
        std::memcpy(&c->wr_cache[i], &bits, 4);   // NaN (a diverged run) compares false below: not in range
    }
}
static ppo_status refresh_weight_range(ppo_ctx* c) {
    if (!c->wrange_dirty || c->gen) return PPO_OK;
    HIPCHK(c, launch_weight_range(B_<float>(c, PPO_BUF_PARAMS), c->L, c->wr_dev, c->wr_host_dev, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->wrange_dirty = false;
    wr_snapshot(c);
    return PPO_OK;
}
// The maxima again, once per update (and after a stand-alone optimizer step): one tiny launch on a stream of its own with NO dependency on the update's
// stream -- it reads whatever the parameters are when it runs (a 32-bit load each; AdamW may be writing them), which is the lag the thresholds' margin
// already covers, and costs the update's stream nothing (as the tail of pack_records_kernel the same sweep cost 7 us per update; inside the AdamW
// kernels, 40 times that).
static ppo_status sweep_weight_range(ppo_ctx* c, hipStream_t s) {
    if (c->gen || c->wrange_dirty) return PPO_OK;   // dirty: the next matrix-core launch recomputes and waits (refresh_weight_range)
    HIPCHK(c, launch_weight_range(B_<float>(c, PPO_BUF_PARAMS), c->L, c->wr_dev, c->wr_host_dev, s));
    return PPO_OK;
}
static inline bool weights_fit_rollout16(const ppo_ctx* c) { return c->wr_cache[PPO_WR_W3] < WR_LIMIT_W3; }
static inline bool weights_fit_update_mfma(const ppo_ctx* c) {
    return c->wr_cache[PPO_WR_W3] < WR_LIMIT_REST && c->wr_cache[PPO_WR_W2] < WR_LIMIT_W2 && c->wr_cache[PPO_WR_REST] < WR_LIMIT_REST;
}
static inline OptGuard opt_guard(const ppo_ctx* c) {
    OptGuard g;
    g.error_flag = c->error_flag;
    return g;
}

// The reference-shape critic on the matrix cores (values_mfma_kernel and the kernels that share its tile body) serves these observation widths; the vector
// critic takes the others.  A context on the generic engine (c->gen) asks neither.
static inline bool critic_is_mfma(const ppo_ctx* c) { return c->O == 4 || c->O == 2; }

// ppo_env_truncation_bootstrap's launch, behind a rollout's critic launches and in front of the scan: the episodes of the rollout just enqueued that the
// time limit cut off get r + gamma V(final observation).  With the switch off the last rollout has no events.  The critic is the one that fills
// PPO_BUF_VALUES: on a fused device env that folds, gen_values' (gauss_fused.hpp: FusedFoldArgs; none of the launches ppo_gauss_fused_launches counts); on
// CartPole / MountainCar, launch_values_mfma for both envs (ppo_internal.hpp: EnvFoldArgs), whatever kernel_flags and the weight range chose for the
// actor -- as in bootstrap_launch, which counts no fall-back either.  envt_on is never set on an env that does not fold (envt_state): a fused env folds
// from PPO_BUF_OBS where its row says so, and every fused env of a PPO_KERNEL_ENV_CUT_STATE context folds from the record (f.cut).
static ppo_status env_fold_truncations(ppo_ctx* c) {
    DevEventList& l = c->env_events;
    if (!c->envt_on) { l.closed = false; return PPO_OK; }
    const ppo_status s = events_clear(c, l);
    if (s != PPO_OK) return s;
    if (c->env) {
        FusedFoldArgs f{};
        f.params = B_<float>(c, PPO_BUF_PARAMS);
        f.obs = B_<float>(c, PPO_BUF_OBS);
        f.actions = c->buf[PPO_BUF_ACTIONS];
        f.fin_len = B_<int32_t>(c, PPO_BUF_FIN_LEN);
        f.B = c->B;
        f.max_episode_steps = c->cfg.max_episode_steps;
        f.gamma = c->cfg.gamma;
        f.rewards = B_<float>(c, PPO_BUF_REWARDS);
        f.cut = c->cut_state;
        events_sink(l, f);
        HIPCHK(c, fused_env_trunc_fold(c->cfg.env_kind, c->gen->L, f, c->stream));
    } else {
        EnvFoldArgs f{};
        f.obs = B_<float>(c, PPO_BUF_OBS);
        f.actions = B_<int32_t>(c, PPO_BUF_ACTIONS);
        f.fin_len = B_<int32_t>(c, PPO_BUF_FIN_LEN);
        f.B = c->B; f.H = c->H;
        f.env_kind = c->cfg.env_kind;
        f.max_episode_steps = c->cfg.max_episode_steps;
        f.gamma = c->cfg.gamma;
        f.rewards = B_<float>(c, PPO_BUF_REWARDS);
        events_sink(l, f);
        HIPCHK(c, launch_env_trunc_fold_mfma(B_<float>(c, PPO_BUF_PARAMS), c->L, f, c->stream));
    }
    return events_close(c, l);
}

// Reward normalisation of a fused device env's rollout (PPO_KERNEL_ENV_REWARD_NORM + ppo_reward_norm_enable; kernels_rewnorm.hip: launch_rewnorm_rollout):
// behind the rollout and its critic launches PPO_BUF_REWARDS [T, N] holds the raw rewards and PPO_BUF_FIN_LEN the dones; rewards never feed back into a
// rollout, so the T per-step updates of a caller-stepped env are three launches here whatever T is (mode 2: one), enqueued without a wait, and they leave the
// bits rn_batch's T launches would.  The episode sums (EP_REW, FIN_REW, the ring) were formed inside the rollout from the raw rewards.  Off: no launch.
static ppo_status env_normalise_rewards(ppo_ctx* c) {
    if (c->rn_mode == 0) return PPO_OK;
    HIPCHK(c, launch_rewnorm_rollout(c->rn_mode, B_<float>(c, PPO_BUF_REWARDS), B_<int32_t>(c, PPO_BUF_FIN_LEN), c->N, c->T, c->rn_ret, c->rn_stats, c->rn_ws,
                                     c->rn_count, c->cfg.gamma, c->rn_eps, c->rn_clip, c->stream));
    if (c->rn_mode == 1)
        for (int t = 0; t < c->T; t++) c->rn_count += (double)c->N;   // step by step, as rn_batch counts (and the merge kernel with it)
    return PPO_OK;
}

// A fused device env: gauss_rollout_kernel / cat_rollout_kernel (all T steps), then gen_rollout's tail -- the critic over the stored observations and over
// NEXT_OBS: three launches; with ppo_env_truncation_bootstrap on (an env that folds only), the fold behind them.  forced: the family's action type, or null
static ppo_status fused_env_rollout(ppo_ctx* c, const void* forced) {
    ppo_status s = consume_finished_episodes(c);
    if (s != PPO_OK) return s;
    FusedRolloutArgs r{};
    r.params = B_<float>(c, PPO_BUF_PARAMS);
    r.N = c->N; r.T = c->T; r.max_episode_steps = c->cfg.max_episode_steps;
    r.seed = c->cfg.seed; r.env_offset = c->cfg.env_offset; r.step_base = c->rollout_steps;
    r.env_state = B_<float>(c, PPO_BUF_ENV_STATE);
    r.ep_len = B_<int32_t>(c, PPO_BUF_EP_LEN);
    r.ep_rew = B_<float>(c, PPO_BUF_EP_REW);
    r.reset_count = B_<int32_t>(c, PPO_BUF_RESET_COUNT);
    r.obs = B_<float>(c, PPO_BUF_OBS);
    r.masks = B_<uint8_t>(c, PPO_BUF_MASKS);
    r.actions = c->buf[PPO_BUF_ACTIONS];
    r.logprobs = B_<float>(c, PPO_BUF_LOGPROBS);
    r.rewards = B_<float>(c, PPO_BUF_REWARDS);
    r.dones = B_<float>(c, PPO_BUF_DONES);
    r.fin_len = B_<int32_t>(c, PPO_BUF_FIN_LEN);
    r.fin_rew = B_<float>(c, PPO_BUF_FIN_REW);
    r.next_obs = B_<float>(c, PPO_BUF_NEXT_OBS);
    r.next_done = B_<int32_t>(c, PPO_BUF_NEXT_DONE);
    r.forced = forced;
    r.cut = c->cut_state;
    {
        ProfScope ps(c, PROF_ROLLOUT);
        HIPCHK(c, launch_fused_env_rollout(c->cfg.env_kind, c->cfg.dist_kind, c->gen->L, r, c->stream));
        s = gen_values(c, r.obs, (int64_t)c->T * c->N, B_<float>(c, PPO_BUF_VALUES));
        if (s == PPO_OK) s = gen_values(c, r.next_obs, c->N, B_<float>(c, PPO_BUF_NEXT_VALUE));
        if (s != PPO_OK) return s;
        s = env_normalise_rewards(c);   // in front of the fold: gamma * V is added to the normalised reward, as on a caller-stepped env
        if (s != PPO_OK) return s;
        s = env_fold_truncations(c);
        if (s != PPO_OK) return s;
    }
    c->rollout_steps += c->T;
    c->global_step += (int64_t)c->T * c->cfg.global_num_envs;
    c->fin_pending = true;
    return PPO_OK;
}

extern "C" ppo_status ppo_rollout_f32(ppo_ctx* c, const float* forced_actions) {
    NEED(c, c != nullptr, "null ctx");
    if (c->host_env) return host_env_refuses(c, "ppo_rollout_f32");
    if (!is_gauss(c)) return wrong_action_type(c, "ppo_rollout_f32", "ppo_rollout");
    DeviceGuard dev_guard(c);
    return fused_env_rollout(c, forced_actions);   // a Gaussian context with a device env is an env of the fused rollout (ppo_ctx_create)
}

extern "C" ppo_status ppo_rollout(ppo_ctx* c, const int64_t* forced_actions) {
    NEED(c, c != nullptr, "null ctx");
    if (c->host_env) return host_env_refuses(c, "ppo_rollout");
    if (is_gauss_env(c)) {
        if (forced_actions) return wrong_action_type(c, "ppo_rollout with forced actions", "ppo_rollout_f32");
        DeviceGuard dev_guard(c);
        return fused_env_rollout(c, nullptr);
    }
    DeviceGuard dev_guard(c);
    if (is_cat_env(c)) return fused_env_rollout(c, forced_actions);
    ppo_status s = consume_finished_episodes(c);
    if (s != PPO_OK) return s;
    if (c->gen && !c->env_generic) return gen_rollout(c, forced_actions);
    // worst case one reset per env per step
    s = ensure_reset_table(c, c->rollout_steps + c->T + 4);
    if (s != PPO_OK) return s;
    if (c->env_generic) return gen_rollout(c, forced_actions);   // PPO_KERNEL_ENV_GENERIC: the same reset table under the generic engine's rollout
    RolloutArgs a{};
    a.params = B_<float>(c, PPO_BUF_PARAMS);
    a.L = c->L;
    a.dist_kind = c->cfg.dist_kind;
    a.env_kind = c->cfg.env_kind;
    a.N = c->N; a.T = c->T;
    a.max_episode_steps = c->cfg.max_episode_steps;
    a.seed = c->cfg.seed; a.env_offset = c->cfg.env_offset; a.step_base = c->rollout_steps;
    a.env_state = B_<float>(c, PPO_BUF_ENV_STATE);
    a.ep_len = B_<int32_t>(c, PPO_BUF_EP_LEN);
    a.ep_rew = B_<float>(c, PPO_BUF_EP_REW);
    a.reset_count = B_<int32_t>(c, PPO_BUF_RESET_COUNT);
    a.reset_table = c->reset_table; a.reset_cap = c->reset_cap; a.error_flag = c->error_flag;
    s = refresh_weight_range(c);
    if (s != PPO_OK) return s;
    a.vector_kernel = c->rollout_vector ? 1 : 0;
    wr_snapshot(c);
    if (!a.vector_kernel && !weights_fit_rollout16(c)) { a.vector_kernel = 1; c->vector_fallback_launches += 1; }
    a.obs = B_<float>(c, PPO_BUF_OBS);
    a.actions = B_<int32_t>(c, PPO_BUF_ACTIONS);
    a.logprobs = B_<float>(c, PPO_BUF_LOGPROBS);
    a.rewards = B_<float>(c, PPO_BUF_REWARDS);
    a.dones = B_<float>(c, PPO_BUF_DONES);
    a.values = B_<float>(c, PPO_BUF_VALUES);
    a.masks = c->cfg.dist_kind == PPO_DIST_MASKED ? B_<uint8_t>(c, PPO_BUF_MASKS) : nullptr;
    a.fin_len = B_<int32_t>(c, PPO_BUF_FIN_LEN);
    a.fin_rew = B_<float>(c, PPO_BUF_FIN_REW);
    a.next_obs = B_<float>(c, PPO_BUF_NEXT_OBS);
    a.next_done = B_<int32_t>(c, PPO_BUF_NEXT_DONE);
    a.next_value = B_<float>(c, PPO_BUF_NEXT_VALUE);
    a.forced_actions = forced_actions;
    bool ring_pushed = false;
    {
        ProfScope ps(c, PROF_ROLLOUT);
        // the critic launch also counts and pushes this rollout's finished episodes (launch_values_ring_mfma) unless PPO_KERNEL_SEPARATE_LAUNCHES asks for
        // the two stand-alone kernels, which then run in front of the next reader (consume_finished_episodes)
        RingFuseArgs rf{};
        rf.fin_len = a.fin_len; rf.fin_rew = a.fin_rew; rf.row_counts = c->row_counts; rf.group_bits = c->group_bits; rf.ring = c->ring;
        rf.ticket = c->pair_tickets; rf.step_base = c->rollout_steps; rf.global_num_envs = c->cfg.global_num_envs; rf.env_offset = c->cfg.env_offset;
        ring_pushed = !c->separate_launches && critic_is_mfma(c);
        HIPCHK(c, launch_rollout(a, c->stream, ring_pushed ? &rf : nullptr));
        s = env_fold_truncations(c);   // (one stream: ppo_calc_advantage and ppo_train_iteration's scan both follow)
        if (s != PPO_OK) return s;
    }
    c->rollout_steps += c->T;
    c->global_step += (int64_t)c->T * c->cfg.global_num_envs;  // global_step += num_envs per step (:526)
    c->fin_pending = !ring_pushed;
    return PPO_OK;
}

// ---------------------------------------------------------------------------------------------------------
// Evaluation (no reference counterpart; the reference's README offers trained policies for inference, its code has only train())
// ---------------------------------------------------------------------------------------------------------
static ppo_status eval_scratch(ppo_ctx* c, int64_t n, int64_t seed) {
    if (n > c->eval_cap) {
        int64_t cap = std::max<int64_t>(c->eval_cap, 1024);
        while (cap < n) cap *= 2;
        float* r = nullptr;
        int32_t* l = nullptr;
        HIPCHK(c, hipStreamSynchronize(c->stream));   // nothing enqueued may still be using the arrays that are replaced
        HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&r), (size_t)cap * sizeof(float)));
        if (hipMalloc(reinterpret_cast<void**>(&l), (size_t)cap * 2 * sizeof(int32_t)) != hipSuccess) {
            (void)hipFree(r);
            return fail(c, PPO_ERR_HIP, "ppo_evaluate: no device memory for %lld episodes", (long long)cap);
        }
        for (void* old : { (void*)c->eval_ret, (void*)c->eval_len })
            if (old) { c->allocs.erase(std::remove(c->allocs.begin(), c->allocs.end(), old), c->allocs.end()); (void)hipFree(old); }
        c->allocs.push_back(r); c->allocs.push_back(l);
        c->eval_ret = r; c->eval_len = l; c->eval_cap = cap;
    }
    if (c->cfg.env_kind != PPO_ENV_CARTPOLE) return PPO_OK;
    if (n > c->eval_table_cap) {
        int64_t cap = std::max<int64_t>(c->eval_table_cap, 1024);
        while (cap < n) cap *= 2;
        float* d = nullptr;
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&d), (size_t)cap * 4 * sizeof(float)));
        if (c->eval_table) { c->allocs.erase(std::remove(c->allocs.begin(), c->allocs.end(), (void*)c->eval_table), c->allocs.end()); (void)hipFree(c->eval_table); }
        c->allocs.push_back(d);
        c->eval_table = d; c->eval_table_cap = cap; c->eval_table_rows = 0;
    }
    if (c->eval_table_rows < n || c->eval_table_seed != seed) {
        // row e of the stream is the same whatever the stream's length (one generator, drawn in order): a table of cap rows serves every n <= cap
        c->eval_table_h.resize((size_t)c->eval_table_cap * 4);
        ppo_cartpole_reset_stream_h(seed, c->eval_table_cap, c->eval_table_h.data());
        HIPCHK(c, hipStreamSynchronize(c->stream));   // a launch of an earlier call may still read the table
        HIPCHK(c, hipMemcpy(c->eval_table, c->eval_table_h.data(), (size_t)c->eval_table_cap * 4 * sizeof(float), hipMemcpyHostToDevice));
        c->eval_table_rows = c->eval_table_cap; c->eval_table_seed = seed;
    }
    return PPO_OK;
}

// ppo_evaluate's launch on CartPole / MountainCar (kernels_rollout.hip: eval16_kernel / evalv_kernel)
static ppo_status eval_launch_categorical(ppo_ctx* c, int64_t n_episodes, int64_t seed, int32_t greedy) {
    ppo_status s = PPO_OK;
    EvalArgs a{};
    a.params = B_<float>(c, PPO_BUF_PARAMS);
    a.L = c->L;
    a.dist_kind = c->cfg.dist_kind;
    a.env_kind = c->cfg.env_kind;
    a.max_episode_steps = c->cfg.max_episode_steps;
    a.greedy = greedy != 0;
    a.n_episodes = n_episodes;
    a.seed = seed;
    a.reset_table = c->eval_table;
    a.ep_return = c->eval_ret;
    a.ep_length = c->eval_len;
    a.ep_trunc = c->eval_len + c->eval_cap;
    // the arithmetic ppo_rollout would choose now, from the same weight-range snapshot; the snapshot is read into locals and the fallback is not counted:
    // the call leaves the training state, ppo_profile.vector_fallback_launches included, as it was
    a.vector_kernel = (c->rollout_vector || !policy_act16_serves(c->L)) ? 1 : 0;
    if (!a.vector_kernel) {
        s = refresh_weight_range(c);
        if (s != PPO_OK) return s;
        const uint32_t bits = __atomic_load_n(c->wr_host + PPO_WR_W3, __ATOMIC_RELAXED);
        float w3;
        std::memcpy(&w3, &bits, 4);
        if (!(w3 < WR_LIMIT_W3)) a.vector_kernel = 1;
    }
    HIPCHK(c, launch_evaluate(a, c->stream));
    return PPO_OK;
}

extern "C" ppo_status ppo_evaluate(ppo_ctx* c, int64_t n_episodes, int64_t seed, int32_t greedy, float* ep_return, int32_t* ep_length, ppo_eval_stats* out_h) {
    NEED(c, c != nullptr, "null ctx");
    if (is_gauss_env(c) && !c->env->evaluates)
        return fail(c, PPO_ERR_UNSUPPORTED, "ppo_evaluate is not built for %s: step the episodes through ppo_policy_act_f32 with greedy = 1 and "
                                            "ppo_env_transition_f32", c->env->name);
    const bool fused_env = c->env && c->env->evaluates;   // the episodes run on the fused kernels (gauss_eval_kernel, cat_eval_kernel); the host side is shared
    if (c->env_generic)
        return fail(c, PPO_ERR_UNSUPPORTED, "ppo_evaluate is not built for PPO_KERNEL_ENV_GENERIC contexts: its episode kernels hold the reference's 2 x 64 network; step "
                                            "the episodes with ppo_policy_act_greedy + ppo_env_transition");
    if (c->host_env || (c->gen && !fused_env) || c->cfg.env_kind == PPO_ENV_SYNTHETIC)
        return fail(c, PPO_ERR_UNSUPPORTED, "ppo_evaluate steps the context's device environment (CartPole, MountainCar); this context's environment is %s: "
                                            "run the episodes on the host with one ppo_policy_act_greedy launch per step",
                    c->host_env ? "the caller's (PPO_ENV_HOST)" : "synthetic (PPO_ENV_SYNTHETIC)");
    NEED(c, out_h != nullptr, "ppo_evaluate: out_h is null");
    NEED(c, n_episodes > 0, "ppo_evaluate: n_episodes <= 0");
    NEED(c, n_episodes < (1ll << 28), "ppo_evaluate: more than 2^28 episodes");
    NEED(c, c->cfg.max_episode_steps > 0, "ppo_evaluate: max_episode_steps <= 0 (an episode would never be truncated)");
    NEED(c, c->O == (fused_env ? c->env->obs : (c->cfg.env_kind == PPO_ENV_CARTPOLE ? 4 : 2)), "ppo_evaluate: obs_size does not match the environment");
    DeviceGuard dev_guard(c);
    ppo_status s = eval_scratch(c, n_episodes, seed);
    if (s != PPO_OK) return s;
    if (fused_env) {
        FusedEvalArgs g{};
        g.params = B_<float>(c, PPO_BUF_PARAMS);
        g.n_episodes = n_episodes; g.seed = seed;
        g.max_episode_steps = c->cfg.max_episode_steps;
        g.greedy = greedy != 0;
        g.ep_return = c->eval_ret; g.ep_length = c->eval_len; g.ep_trunc = c->eval_len + c->eval_cap;
        HIPCHK(c, fused_env_evaluate(c->cfg.env_kind, c->cfg.dist_kind, c->gen->L, g, c->stream));
    } else {
        s = eval_launch_categorical(c, n_episodes, seed, greedy);
        if (s != PPO_OK) return s;
    }
    if (ep_return) HIPCHK(c, hipMemcpyAsync(ep_return, c->eval_ret, (size_t)n_episodes * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    if (ep_length) HIPCHK(c, hipMemcpyAsync(ep_length, c->eval_len, (size_t)n_episodes * sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream));
    std::vector<float> ret((size_t)n_episodes);
    std::vector<int32_t> len((size_t)n_episodes), trunc((size_t)n_episodes);
    HIPCHK(c, hipMemcpyAsync(ret.data(), c->eval_ret, ret.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(len.data(), c->eval_len, len.size() * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(trunc.data(), c->eval_len + c->eval_cap, trunc.size() * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // the summary: f64, in index order
    ppo_eval_stats o{};
    o.episodes = n_episodes;
    double rs = 0.0, ls = 0.0;
    o.return_min = o.return_max = ret[0];
    o.length_min = o.length_max = len[0];
    for (int64_t i = 0; i < n_episodes; i++) {
        rs += (double)ret[i];
        ls += (double)len[i];
        o.env_steps += len[i];
        o.return_min = std::min(o.return_min, (double)ret[i]);
        o.return_max = std::max(o.return_max, (double)ret[i]);
        o.length_min = std::min<int64_t>(o.length_min, len[i]);
        o.length_max = std::max<int64_t>(o.length_max, len[i]);
        o.truncated += trunc[i] != 0;
    }
    o.return_mean = rs / (double)n_episodes;
    o.length_mean = ls / (double)n_episodes;
    double q = 0.0;
    for (int64_t i = 0; i < n_episodes; i++) { const double d = (double)ret[i] - o.return_mean; q += d * d; }
    o.return_std = std::sqrt(q / (double)n_episodes);
    *out_h = o;
    return PPO_OK;
}

// Stateless Linear-layer product on the matrix cores (kernels_gemm.hip).
extern "C" ppo_status ppo_matmul(int32_t trans_a, int32_t trans_b, int64_t M, int64_t N, int64_t K, const float* a, int64_t lda, const float* b, int64_t ldb,
                                 float* c, int64_t ldc, int32_t epilogue, const float* aux, int64_t ld_aux, int32_t precision, void* stream) {
    if (!a || !b || !c || M < 0 || N < 0 || K < 0 || epilogue < PPO_MM_EPI_NONE || epilogue > PPO_MM_EPI_DTANH) return PPO_ERR_INVALID;
    if (epilogue != PPO_MM_EPI_NONE && !aux) return PPO_ERR_INVALID;
    if (precision != PPO_MM_F32X3 && precision != PPO_MM_BF16) return PPO_ERR_INVALID;
    return launch_matmul(trans_a != 0, trans_b != 0, M, N, K, a, lda, b, ldb, c, ldc, epilogue, aux, ld_aux, precision, 1, 0, nullptr, 0, nullptr, 0, 0, (hipStream_t)stream) == hipSuccess
               ? PPO_OK : PPO_ERR_HIP;
}
extern "C" ppo_status ppo_gae(const float* rewards, const float* values, const float* dones, const float* next_value, const int32_t* next_done,
                              int64_t T, int64_t N, float gamma, float gae_lambda, float* advantages, float* returns, void* stream) {
    if (!rewards || !values || !dones || !next_value || !next_done || !advantages || !returns || T < 0 || N < 0) return PPO_ERR_INVALID;
    return launch_gae(rewards, values, dones, next_value, next_done, T, N, gamma, gae_lambda, advantages, returns, nullptr, (hipStream_t)stream) == hipSuccess ? PPO_OK : PPO_ERR_HIP;
}
extern "C" ppo_status ppo_gae_fast(const float* rewards, const float* values, const float* dones, const float* next_value, const int32_t* next_done,
                                   int64_t T, int64_t N, float gamma, float gae_lambda, float* advantages, float* returns, void* stream) {
    if (!rewards || !values || !dones || !next_value || !next_done || !advantages || !returns || T < 0 || N < 0) return PPO_ERR_INVALID;
    return launch_gae_fast(rewards, values, dones, next_value, next_done, T, N, gamma, gae_lambda, advantages, returns, (hipStream_t)stream) == hipSuccess ? PPO_OK : PPO_ERR_HIP;
}
extern "C" ppo_status ppo_nstep_returns(const float* rewards, const float* values, const float* dones, const float* next_value,
                                        const int32_t* next_done, int64_t T, int64_t N, float gamma, float* advantages, float* returns, void* stream) {
    if (!rewards || !values || !dones || !next_value || !next_done || !advantages || !returns || T < 0 || N < 0) return PPO_ERR_INVALID;
    return launch_nstep(rewards, values, dones, next_value, next_done, T, N, gamma, advantages, returns, nullptr, (hipStream_t)stream) == hipSuccess ? PPO_OK : PPO_ERR_HIP;
}

// K4 on the context's buffers: GAE (PPO_Discrete.cpp:283-306) or n-step returns (:309-329) by cfg.use_gae.
static ppo_status run_scan(ppo_ctx* c) {
    ProfScope ps(c, PROF_GAE);
    if (c->cfg.use_gae)
        HIPCHK(c, launch_gae(B_<float>(c, PPO_BUF_REWARDS), B_<float>(c, PPO_BUF_VALUES), B_<float>(c, PPO_BUF_DONES), B_<float>(c, PPO_BUF_NEXT_VALUE),
                             B_<int32_t>(c, PPO_BUF_NEXT_DONE), c->T, c->N, c->cfg.gamma, c->cfg.gae_lambda, B_<float>(c, PPO_BUF_ADVANTAGES),
                             B_<float>(c, PPO_BUF_RETURNS), c->error_flag, c->stream));
    else
        HIPCHK(c, launch_nstep(B_<float>(c, PPO_BUF_REWARDS), B_<float>(c, PPO_BUF_VALUES), B_<float>(c, PPO_BUF_DONES), B_<float>(c, PPO_BUF_NEXT_VALUE),
                               B_<int32_t>(c, PPO_BUF_NEXT_DONE), c->T, c->N, c->cfg.gamma, B_<float>(c, PPO_BUF_ADVANTAGES),
                               B_<float>(c, PPO_BUF_RETURNS), c->error_flag, c->stream));
    return PPO_OK;
}

extern "C" ppo_status ppo_calc_advantage(ppo_ctx* c) {
    NEED(c, c != nullptr, "null ctx");
    DeviceGuard dev_guard(c);
    // bootstrap value if not done: next_value = Critic(next_obs) (PPO_Discrete.cpp:280)
    const ppo_status s = ppo_get_value(c, B_<float>(c, PPO_BUF_NEXT_OBS), c->N, B_<float>(c, PPO_BUF_NEXT_VALUE));
    if (s != PPO_OK) return s;
    return run_scan(c);
}

// ---------------------------------------------------------------------------------------------------------
// Update
// ---------------------------------------------------------------------------------------------------------
extern "C" ppo_status ppo_generate_permutations(ppo_ctx* c) {
    NEED(c, c != nullptr, "null ctx");
    DeviceGuard dev_guard(c);
    HIPCHK(c, launch_permutations(B_<int32_t>(c, PPO_BUF_PERM), c->B, c->cfg.update_epochs, c->cfg.seed, c->updates, c->rank, c->stream));
    return PPO_OK;
}

// AdamW scalars exactly as LibTorch forms them on the host (optim/adamw.cpp): doubles narrowed to float at use.
static AdamCoef adam_coef(double lr, int64_t t) {
    const double beta1 = 0.9, beta2 = 0.999, wd = 1e-2;
    const double bc1 = 1.0 - std::pow(beta1, (double)t), bc2 = 1.0 - std::pow(beta2, (double)t);
    AdamCoef k;
    k.decay = (float)(1.0 - lr * wd);
    k.neg_step = (float)(-(lr / bc1));
    k.sqrt_bc2 = (float)std::sqrt(bc2);
    k.pad = 0.0f;
    return k;
}

static ppo_status allreduce_sum(ppo_ctx* c, void* buf, size_t count, bool f64) {
    if (c->world <= 1 && !c->force_collectives) return PPO_OK;
    // bracketed like the dominant kernel: every call in mode 1, otherwise the one that follows a bracketed update launch
    ProfScope ps(c, PROF_ALLREDUCE, c->prof_every <= 1 || c->prof_last_sampled);
    c->prof_last_sampled = false;
    if (c->xchg) {
        ExchangeComm& x = *c->xchg;
        const size_t bytes = count * (f64 ? 8 : 4);
        NEED(c, bytes <= x.slot_bytes, "all-reduce payload exceeds the exchange slot");
        XchgPtrs pp{};
        for (int r = 0; r < c->world; r++) pp.p[r] = x.peer[r];
        x.seq += 1;
        HIPCHK(c, launch_exchange_allreduce(buf, count, f64, pp, c->rank, c->world, x.slot_bytes, x.seq, x.timeout_flag, c->stream));
        return PPO_OK;
    }
    if (c->lgroup) {
        LocalGroup* g = c->lgroup.get();
        HIPCHK(c, hipEventRecord(c->lg_ready, c->stream));
        uint64_t my_gen;
        hipError_t he = hipSuccess;
        bool failed = false;
        {
            std::unique_lock<std::mutex> lk(g->mu);
            if (g->failed) return fail(c, PPO_ERR_COMM, "in-process group has failed");
            g->bufs[c->rank] = buf;
            g->ready[c->rank] = c->lg_ready;
            my_gen = g->generation;
            if (++g->arrived == g->n) {
                // last arriver: one kernel on its stream reads every rank's buffer.  Whatever happens here, the generation advances and everybody is
                // woken: a failure is reported to all members instead of leaving them in cv.wait
                for (int r = 0; r < g->n && he == hipSuccess; r++) he = hipStreamWaitEvent(c->stream, g->ready[r], 0);
                PtrPack pk{};
                for (int r = 0; r < g->n; r++) pk.p[r] = g->bufs[r];
                if (he == hipSuccess) he = launch_local_allreduce(pk, g->n, count, f64, c->stream);
                if (he == hipSuccess) he = hipEventRecord(g->done[my_gen & 1], c->stream);
                if (he != hipSuccess) g->failed = true;
                g->arrived = 0;
                g->generation++;
                g->cv.notify_all();
            } else {
                g->cv.wait(lk, [&] { return g->generation != my_gen; });
            }
            failed = g->failed;
        }
        if (he != hipSuccess) return fail(c, PPO_ERR_HIP, "in-process all-reduce failed: %s", hipGetErrorString(he));
        if (failed) return fail(c, PPO_ERR_COMM, "in-process all-reduce failed on another member of the group");
        HIPCHK(c, hipStreamWaitEvent(c->stream, g->done[my_gen & 1], 0));
        return PPO_OK;
    }
    const int rc = rccl::AllReduce(buf, buf, count, f64 ? rccl::kFloat64 : rccl::kFloat32, rccl::kSum, c->comm, c->stream);
    if (rc != 0) return fail(c, PPO_ERR_COMM, "ncclAllReduce failed: %s", rccl::GetErrorString ? rccl::GetErrorString(rc) : "?");
    return PPO_OK;
}

// ---- generic networks: one minibatch step = gather, two forward passes that keep their activations, loss, two backward passes ----
static ppo_status gen_fwd_bwd(ppo_ctx* c, const int32_t* idx, int64_t M, int slot) {
    GenericCtx& g = *c->gen;
    const GenLayout& GL = g.L;
    NEED(c, M >= 1 && M <= g.rows_max, "minibatch larger than the workspace");
    const double global_M = (double)M * c->world;
    c->last_global_M = global_M;
    float* params = B_<float>(c, PPO_BUF_PARAMS);
    float* grads = B_<float>(c, PPO_BUF_GRADS);
    if (c->gauss_fused || c->cat_fused) {
        // PPO_KERNEL_GAUSS_FUSED / PPO_KERNEL_CAT_FUSED: gather, both nets' forward, loss and backward in one launch, the slab sums in a second; behind them
        // the engine's own loss sums, all-reduce, norm and AdamW
        {
            ProfScope ps(c, PROF_FWD_BWD);
            c->gen_opt_fused_ok = false;
            c->gen_pre_idx = nullptr;
            c->gf_launches[2] += 1;
            if (c->cat_fused)
                HIPCHK(c, cat_fused_fwd_bwd(GL, c->hp, params, B_<float>(c, PPO_BUF_OBS), B_<int32_t>(c, PPO_BUF_ACTIONS), B_<uint8_t>(c, PPO_BUF_MASKS),
                                            B_<float>(c, PPO_BUF_LOGPROBS), B_<float>(c, PPO_BUF_ADVANTAGES), B_<float>(c, PPO_BUF_RETURNS), B_<float>(c, PPO_BUF_VALUES), idx, M,
                                            1.0 / global_M, global_M, c->cfg.norm_adv ? c->adv_stats + (size_t)slot * PPO_ADV_PARTS : nullptr, c->gf_slab, g.loss_part, grads,
                                            c->stream));
            else
                HIPCHK(c, gauss_fused_fwd_bwd(GL, c->hp, params, B_<float>(c, PPO_BUF_OBS), B_<float>(c, PPO_BUF_ACTIONS), B_<float>(c, PPO_BUF_LOGPROBS),
                                              B_<float>(c, PPO_BUF_ADVANTAGES), B_<float>(c, PPO_BUF_RETURNS), B_<float>(c, PPO_BUF_VALUES), idx, M, 1.0 / global_M, global_M,
                                              c->cfg.norm_adv ? c->adv_stats + (size_t)slot * PPO_ADV_PARTS : nullptr, c->gf_slab, g.loss_part, grads, c->stream));
        }
        ProfScope ps(c, PROF_REDUCE);
        HIPCHK(c, gen_loss_sums(g, c->loss_sums, grads + GL.P, c->stream));
        return PPO_OK;
    }
    {
        ProfScope ps(c, PROF_FWD_BWD);
        // Both fused passes available (bf16 storage, widths the kernels are built for): the two nets share every launch -- forward, each layer's backward, the
        // slab sums -- on ONE stream: the second net's workgroups take the CUs the first net's leave (forward) or run beside them on the other half of the
        // chip (backward), with no fork / join events between the streams (four per step, several us each).  Otherwise: the critic's passes on a second stream.
        const bool classic = (c->cfg.kernel_flags & PPO_KERNEL_GENERIC_CLASSIC) != 0;   // the step's first form (ppo_hip.h): A/B runs and tests
        const bool paired = !classic && g.bf16 && gen_fused_forward_ok(g) && gen_fused_backward_ok(g) && M <= GEN_FUSED_MAX_ROWS;
        const bool paired_bwd = paired;
        const bool two = !paired && g.bf16 && c->stream2 != nullptr;   // a kernel of one net fills the CUs the other net's kernel is draining
        const bool two_bwd = !paired_bwd && g.bf16 && c->stream2 != nullptr;
        auto gather = [&](const int32_t* rows, int64_t n, hipStream_t st) {
            return gen_gather(GL, B_<float>(c, PPO_BUF_OBS), B_<int32_t>(c, PPO_BUF_ACTIONS), GL.gauss ? nullptr : B_<uint8_t>(c, PPO_BUF_MASKS), B_<float>(c, PPO_BUF_LOGPROBS),
                              B_<float>(c, PPO_BUF_ADVANTAGES), B_<float>(c, PPO_BUF_RETURNS), B_<float>(c, PPO_BUF_VALUES), rows, n, g, st);
        };
        // the fused kernels read the minibatch's rows in place (generic.hpp: GenericCtx::obs_bf, rows_idx); the observations are rounded once per update --
        // a stand-alone step (whose caller may have rewritten the buffers) rounds them every time
        const bool in_place = !classic && g.bf16 && g.obs_bf && gen_fused_forward_ok(g) && gen_fused_backward_ok(g) && M <= GEN_FUSED_MAX_ROWS;
        g.rows_idx = nullptr;
        g.rows_rec = nullptr;
        if (in_place) {
            g.rows_src = GenRowSrc{ B_<int32_t>(c, PPO_BUF_ACTIONS), c->cfg.dist_kind == PPO_DIST_MASKED ? B_<uint8_t>(c, PPO_BUF_MASKS) : nullptr, B_<float>(c, PPO_BUF_LOGPROBS),
                                    B_<float>(c, PPO_BUF_ADVANTAGES), B_<float>(c, PPO_BUF_RETURNS), B_<float>(c, PPO_BUF_VALUES) };
            if (!c->gen_obs_bf_valid) {
                // inside ppo_update: the whole batch once, valid for all of the update's steps.  A stand-alone step (its caller may have rewritten any buffer
                // since the last one): only the step's own M rows, in place -- not all B of them for a step that reads a few
                const bool whole = c->wr_in_update;
                HIPCHK(c, launch_to_bf16_pad(B_<float>(c, PPO_BUF_OBS), whole ? c->B : M, GL.obs, g.obs_bf, g.ld_in0, c->stream, whole ? nullptr : idx));
                if (g.row_rec) HIPCHK(c, gen_pack_rows(GL, g.rows_src, whole ? c->B : M, g.row_rec, c->stream, whole ? nullptr : idx));
                c->gen_obs_bf_valid = whole;
            }
            g.rows_idx = idx;
            g.rows_rec = reinterpret_cast<const float4*>(g.row_rec);
        } else if (two && c->gen_pre_idx == idx && c->gen_pre_M == M) {
            HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_gather, 0));   // gathered ahead by the step before
        } else {
            HIPCHK(c, gather(idx, M, c->stream));
        }
        c->gen_pre_idx = nullptr;
        auto fork = [&]() -> hipError_t { const hipError_t e = hipEventRecord(c->ev_fork, c->stream); return e != hipSuccess ? e : hipStreamWaitEvent(c->stream2, c->ev_fork, 0); };
        auto join = [&]() -> hipError_t { const hipError_t e = hipEventRecord(c->ev_join, c->stream2); return e != hipSuccess ? e : hipStreamWaitEvent(c->stream, c->ev_join, 0); };
        hipStream_t s0 = two ? c->stream2 : c->stream;
        if (two && g.planes_dirty) { HIPCHK(c, gen_weight_planes(g, params, c->stream)); g.planes_dirty = false; }   // shared by both nets: before the fork
        if (two) HIPCHK(c, fork());
        const uint16_t* x0 = in_place ? g.obs_bf : g.xin_bf;
        // heads + loss + the head layers' backward in the forward launch's epilogue (kernels_generic_fused.hip: FusedLossArgs) where the shape allows
        g.head_fused = 0;
        const bool head_fused = paired && in_place && g.rows_rec != nullptr && !(c->cfg.kernel_flags & PPO_KERNEL_GENERIC_SPLIT_HEAD) && gen_fused_loss_ok(g, M);
        if (head_fused) {
            HIPCHK(c, gen_fused_forward_loss(g, params, x0, g.ld_in0, M, c->hp, 1.0 / global_M, global_M, c->cfg.norm_adv ? c->adv_stats + (size_t)slot * PPO_ADV_PARTS : nullptr,
                                             g.rows_idx, c->stream));
        } else if (paired) {
            HIPCHK(c, gen_fused_forward_both(g, params, x0, g.ld_in0, M, g.logits, g.val, c->stream, g.rows_idx));
        } else if (gen_fused_forward_ok(g) && M <= GEN_FUSED_MAX_ROWS) {   // bf16 storage: each net's forward pass is one launch that also leaves its hidden activations
            HIPCHK(c, gen_fused_forward(g, params, 1, nullptr, x0, g.ld_in0, M, true, g.logits, c->stream, g.rows_idx));
            HIPCHK(c, gen_fused_forward(g, params, 0, nullptr, x0, g.ld_in0, M, true, g.val, s0, g.rows_idx));
        } else {
            HIPCHK(c, gen_forward(g, params, 1, g.xin, M, g.acts[1], nullptr, nullptr, g.logits, c->stream));
            HIPCHK(c, gen_forward(g, params, 0, g.xin, M, g.acts[0], nullptr, nullptr, g.val, s0));
        }
        if (two) HIPCHK(c, join());   // the loss reads the logits and the values
        if (GL.gauss)   // Gaussian policies: their own loss kernel; d(loss)/d(log_std) goes straight to its place behind the actor's layers
            HIPCHK(c, gen_gauss_loss(GL, c->hp, g, params + GL.logstd_off, M, 1.0 / global_M, global_M, c->cfg.norm_adv ? c->adv_stats + (size_t)slot * PPO_ADV_PARTS : nullptr,
                                     grads + GL.logstd_off, c->stream));
        else if (!head_fused) HIPCHK(c, gen_loss(GL, c->hp, g, M, 1.0 / global_M, global_M, c->cfg.norm_adv ? c->adv_stats + (size_t)slot * PPO_ADV_PARTS : nullptr, c->stream));
        // backward: paired too (A/B in one call, configs[4] share: 0.621 ms per optimizer step paired, 0.644 with the backward passes on two streams, 0.683 for
        // round 5's first form -- two streams throughout, gathered copies, four optimizer launches)
        if (two_bwd) HIPCHK(c, fork());
        c->gen_opt_fused_ok = false;
        if (paired_bwd) {
            HIPCHK(c, gen_backward_both(g, params, M, grads, c->stream));
        } else {
            hipStream_t sb = two_bwd ? c->stream2 : c->stream;
            HIPCHK(c, gen_backward(g, params, 1, g.xin, M, g.dlogits, grads, c->stream, two_bwd));
            HIPCHK(c, gen_backward(g, params, 0, g.xin, M, g.dval, grads, sb, two_bwd));
        }
        c->gen_opt_fused_ok = !classic && g.sq_valid[0] && g.sq_valid[1] && c->world == 1 && !c->force_collectives;   // nothing changes the gradient between the slab sums and the optimizer
        if (two_bwd) HIPCHK(c, join());   // the flat gradient is complete
        if (two && c->gen_next_idx && !in_place) {
            // nothing reads this step's gathered rows any more: the next step's gather (42 us of HBM streaming) runs on the second stream beside the
            // loss sums, the all-reduce, the norm, AdamW and the weight planes -- small kernels, one after the other, that leave the chip idle.
            // (Requested at the START of the step instead, into a second set of buffers, it does not overlap at all: its 16 k small workgroups take
            // every CU slot that frees up and the forward pass's one-per-CU workgroups start when it has drained -- measured, same time as no
            // gather-ahead.)
            HIPCHK(c, fork());
            HIPCHK(c, gather(c->gen_next_idx, c->gen_next_M, c->stream2));
            HIPCHK(c, hipEventRecord(c->ev_gather, c->stream2));
            c->gen_pre_idx = c->gen_next_idx; c->gen_pre_M = c->gen_next_M;
        }
    }
    if (!c->gen_opt_fused_ok) {   // (the fused optimizer launch adds the loss kernel's block sums itself)
        ProfScope ps(c, PROF_REDUCE);
        HIPCHK(c, gen_loss_sums(g, c->loss_sums, grads + GL.P, c->stream));
    }
    return PPO_OK;
}

// the T-step rollout as T x { actor GEMMs + heads, stores, env step } and one critic batch at the end (PPO_MultiDiscrete.cpp:547-575)
static ppo_status gen_rollout(ppo_ctx* c, const int64_t* forced) {
    GenericCtx& g = *c->gen;
    const GenLayout& GL = g.L;
    const int N = c->N;
    float* params = B_<float>(c, PPO_BUF_PARAMS);
    float* next_obs = B_<float>(c, PPO_BUF_NEXT_OBS);
    const uint8_t* mask = c->cfg.dist_kind == PPO_DIST_MASKED ? c->cur_mask : nullptr;
    if (c->env_generic) {
        // PPO_KERNEL_ENV_GENERIC: the same plan around CartPole / MountainCar.  The env's masks are all ones (cur_mask, filled once), and PPO_BUF_MASKS is held as
        // the reference-shape rollout holds it: ones under PPO_DIST_MASKED, untouched otherwise
        uint8_t* masks_t = mask ? B_<uint8_t>(c, PPO_BUF_MASKS) : nullptr;
        ProfScope ps(c, PROF_ROLLOUT);
        if (gen_fused_ok(g)) {   // bf16 storage: all T steps in ONE launch (generic_env_rollout_kernel)
            GenEnvRolloutArgs r{};
            r.env_kind = c->cfg.env_kind; r.dist_kind = c->cfg.dist_kind; r.N = N; r.T = c->T; r.max_episode_steps = c->cfg.max_episode_steps;
            r.seed = c->cfg.seed; r.env_offset = c->cfg.env_offset; r.step_base = c->rollout_steps;
            r.env_state = B_<float>(c, PPO_BUF_ENV_STATE); r.ep_len = B_<int32_t>(c, PPO_BUF_EP_LEN); r.ep_rew = B_<float>(c, PPO_BUF_EP_REW);
            r.reset_count = B_<int32_t>(c, PPO_BUF_RESET_COUNT); r.reset_table = c->reset_table; r.reset_cap = c->reset_cap; r.error_flag = c->error_flag;
            r.obs = B_<float>(c, PPO_BUF_OBS); r.masks = masks_t; r.actions = B_<int32_t>(c, PPO_BUF_ACTIONS); r.logprobs = B_<float>(c, PPO_BUF_LOGPROBS);
            r.rewards = B_<float>(c, PPO_BUF_REWARDS); r.dones = B_<float>(c, PPO_BUF_DONES); r.fin_len = B_<int32_t>(c, PPO_BUF_FIN_LEN);
            r.fin_rew = B_<float>(c, PPO_BUF_FIN_REW); r.next_obs = next_obs; r.next_done = B_<int32_t>(c, PPO_BUF_NEXT_DONE); r.forced = forced;
            HIPCHK(c, gen_fused_env_rollout(g, params, r, c->stream));
        } else {
            for (int t = 0; t < c->T; t++) {   // per step: ppo_policy_act's launches (forward, heads), the stores, ppo_env_step's kernel on the context's buffers
                const size_t tn = (size_t)t * N;
                HIPCHK(c, gen_forward(g, params, 1, next_obs, N, nullptr, g.dz[0], g.dz[1], g.logits, c->stream));
                HIPCHK(c, gen_heads(GL, c->cfg.dist_kind, g.logits, mask, forced ? forced + tn * GL.n_heads : nullptr, N, c->cfg.seed, c->cfg.env_offset,
                                    c->rollout_steps + t, g.act64, g.step_lp, g.step_en, c->stream));
                HIPCHK(c, gen_store_step(GL, N, next_obs, mask, g.act64, g.step_lp, B_<int32_t>(c, PPO_BUF_NEXT_DONE), B_<float>(c, PPO_BUF_OBS) + tn * GL.obs,
                                         masks_t ? masks_t + tn * GL.act : nullptr, B_<int32_t>(c, PPO_BUF_ACTIONS) + tn * GL.n_heads, B_<float>(c, PPO_BUF_LOGPROBS) + tn,
                                         B_<float>(c, PPO_BUF_DONES) + tn, c->stream));
                HIPCHK(c, launch_env_step(c->cfg.env_kind, N, c->H, c->cfg.max_episode_steps, c->cfg.seed, c->cfg.env_offset, B_<float>(c, PPO_BUF_ENV_STATE),
                                          B_<int32_t>(c, PPO_BUF_EP_LEN), B_<float>(c, PPO_BUF_EP_REW), B_<int32_t>(c, PPO_BUF_RESET_COUNT), c->reset_table, c->reset_cap,
                                          g.act64, next_obs, B_<float>(c, PPO_BUF_REWARDS) + tn, B_<int32_t>(c, PPO_BUF_NEXT_DONE), c->error_flag, c->stream,
                                          B_<int32_t>(c, PPO_BUF_FIN_LEN) + tn, B_<float>(c, PPO_BUF_FIN_REW) + tn));
            }
        }
        ppo_status s = gen_values(c, B_<float>(c, PPO_BUF_OBS), (int64_t)c->T * N, B_<float>(c, PPO_BUF_VALUES));
        if (s == PPO_OK) s = gen_values(c, next_obs, N, B_<float>(c, PPO_BUF_NEXT_VALUE));
        if (s != PPO_OK) return s;
    } else if (gen_fused_ok(g)) {
        // bf16 storage: the T steps { observation, actor, heads, stores, env transition } in ONE launch, then the critic over all stored observations
        ProfScope ps(c, PROF_ROLLOUT);
        HIPCHK(c, gen_fused_rollout(g, params, c->cfg.dist_kind, N, c->T, c->cfg.max_episode_steps, c->cfg.seed, c->cfg.env_offset, c->rollout_steps,
                                    B_<int32_t>(c, PPO_BUF_EP_LEN), B_<float>(c, PPO_BUF_EP_REW), B_<float>(c, PPO_BUF_OBS), B_<uint8_t>(c, PPO_BUF_MASKS),
                                    B_<int32_t>(c, PPO_BUF_ACTIONS), B_<float>(c, PPO_BUF_LOGPROBS), B_<float>(c, PPO_BUF_REWARDS), B_<float>(c, PPO_BUF_DONES),
                                    B_<int32_t>(c, PPO_BUF_FIN_LEN), B_<float>(c, PPO_BUF_FIN_REW), next_obs, B_<int32_t>(c, PPO_BUF_NEXT_DONE), c->cur_mask, forced,
                                    c->stream));
        ppo_status s = gen_values(c, B_<float>(c, PPO_BUF_OBS), (int64_t)c->T * N, B_<float>(c, PPO_BUF_VALUES));
        if (s == PPO_OK) s = gen_values(c, next_obs, N, B_<float>(c, PPO_BUF_NEXT_VALUE));
        if (s != PPO_OK) return s;
    } else {
        ProfScope ps(c, PROF_ROLLOUT);
        for (int t = 0; t < c->T; t++) {
            const size_t tn = (size_t)t * N;
            const int64_t step = c->rollout_steps + t;
            HIPCHK(c, gen_forward(g, params, 1, next_obs, N, nullptr, g.dz[0], g.dz[1], g.logits, c->stream));
            HIPCHK(c, gen_heads(GL, c->cfg.dist_kind, g.logits, mask, forced ? forced + tn * GL.n_heads : nullptr, N, c->cfg.seed, c->cfg.env_offset, step,
                                g.act64, g.step_lp, g.step_en, c->stream));
            HIPCHK(c, gen_store_step(GL, N, next_obs, mask /* plain Categorical: masks are stored as all ones */, g.act64, g.step_lp, B_<int32_t>(c, PPO_BUF_NEXT_DONE), B_<float>(c, PPO_BUF_OBS) + tn * GL.obs,
                                     B_<uint8_t>(c, PPO_BUF_MASKS) + tn * GL.act, B_<int32_t>(c, PPO_BUF_ACTIONS) + tn * GL.n_heads,
                                     B_<float>(c, PPO_BUF_LOGPROBS) + tn, B_<float>(c, PPO_BUF_DONES) + tn, c->stream));
            HIPCHK(c, gen_synthetic_step(GL, N, c->cfg.seed, c->cfg.env_offset, step, c->cfg.max_episode_steps, B_<int32_t>(c, PPO_BUF_EP_LEN),
                                         B_<float>(c, PPO_BUF_EP_REW), next_obs, c->cur_mask, B_<float>(c, PPO_BUF_REWARDS) + tn,
                                         B_<int32_t>(c, PPO_BUF_NEXT_DONE), B_<int32_t>(c, PPO_BUF_FIN_LEN) + tn, B_<float>(c, PPO_BUF_FIN_REW) + tn, c->stream));
        }
        ppo_status s = gen_values(c, B_<float>(c, PPO_BUF_OBS), (int64_t)c->T * N, B_<float>(c, PPO_BUF_VALUES));
        if (s == PPO_OK) s = gen_values(c, next_obs, N, B_<float>(c, PPO_BUF_NEXT_VALUE));
        if (s != PPO_OK) return s;
    }
    c->rollout_steps += c->T;
    c->global_step += (int64_t)c->T * c->cfg.global_num_envs;
    c->fin_pending = true;
    return PPO_OK;
}

// The matrix-core update kernel gathers from one packed record per sample and net: (re)build them from the flattened rollout buffers
// (PPO_Discrete.cpp:557-562).  Also leaves the explained-variance partial sums (:647-648), which read the same returns / values.
// with_perm (ppo_update with norm_adv, unless PPO_KERNEL_SEPARATE_LAUNCHES): the same launch also forms the update's permutations and advantage sums, and
// with fold_norm (a context that is not sharded) the normalisations of every minibatch slot and the reset of the clip-fraction accumulator
// (launch_pack_perm_stats)
static ppo_status pack_records(ppo_ctx* c, bool with_perm = false, bool fold_norm = false) {
    if (!c->use_mfma || c->gen) return PPO_OK;
    // the observation's fp16 range is an error only where the wave-specialised matrix-core kernel will read the records: not with the one-wave kernel, and
    // not in an update whose weights send every launch to the vector kernel (the caller has refreshed the range snapshot: ppo_update, stand-alone step)
    const bool ws_will_run = !c->update_single_wave && weights_fit_update_mfma(c);
    if (with_perm) {
        PackPermArgs a{};
        a.actions = B_<int32_t>(c, PPO_BUF_ACTIONS); a.n_heads = c->L.n_heads;
        a.masks = c->cfg.dist_kind == PPO_DIST_MASKED ? B_<uint8_t>(c, PPO_BUF_MASKS) : nullptr; a.A = c->L.act;
        a.logprobs = B_<float>(c, PPO_BUF_LOGPROBS); a.returns = B_<float>(c, PPO_BUF_RETURNS); a.values = B_<float>(c, PPO_BUF_VALUES);
        a.rec_critic = reinterpret_cast<float4*>(c->rec_critic); a.rec_actor = reinterpret_cast<float4*>(c->rec_actor);
        a.ev_out = c->ev_sums; a.error_flag = ws_will_run ? c->error_flag : nullptr;
        a.update_index = c->updates; a.rank_salt = c->rank; a.stat_out = c->adv_stats;
        a.n_slots = c->cfg.update_epochs * c->n_mb;
        a.norm_out = fold_norm ? c->adv_norm : nullptr; a.zero2 = fold_norm ? c->clipfrac_accum : nullptr; a.ticket = c->pair_tickets + 1;
        HIPCHK(c, launch_pack_perm_stats(c->L, B_<float>(c, PPO_BUF_OBS), B_<float>(c, PPO_BUF_ADVANTAGES), B_<int32_t>(c, PPO_BUF_PERM), c->B,
                                         c->cfg.update_epochs, c->MB, c->cfg.seed, a, c->stream));
        return PPO_OK;
    }
    HIPCHK(c, launch_pack_records(c->L, B_<float>(c, PPO_BUF_OBS), B_<int32_t>(c, PPO_BUF_ACTIONS),
                                  c->cfg.dist_kind == PPO_DIST_MASKED ? B_<uint8_t>(c, PPO_BUF_MASKS) : nullptr, B_<float>(c, PPO_BUF_LOGPROBS),
                                  B_<float>(c, PPO_BUF_ADVANTAGES), B_<float>(c, PPO_BUF_RETURNS), B_<float>(c, PPO_BUF_VALUES), c->B, c->rec_critic,
                                  c->rec_actor, c->ev_sums, ws_will_run ? c->error_flag : nullptr, c->stream));
    return PPO_OK;
}

static ppo_status fwd_bwd(ppo_ctx* c, const int32_t* idx, int64_t M, int slot, bool reduce = true) {
    if (c->gen) return gen_fwd_bwd(c, idx, M, slot);
    UpdateArgs a{};
    a.params = B_<float>(c, PPO_BUF_PARAMS);
    a.L = c->L;
    a.hp = c->hp;
    a.obs = B_<float>(c, PPO_BUF_OBS);
    a.actions = B_<int32_t>(c, PPO_BUF_ACTIONS);
    a.masks = c->cfg.dist_kind == PPO_DIST_MASKED ? B_<uint8_t>(c, PPO_BUF_MASKS) : nullptr;
    a.logprobs = B_<float>(c, PPO_BUF_LOGPROBS);
    a.advantages = B_<float>(c, PPO_BUF_ADVANTAGES);
    a.returns = B_<float>(c, PPO_BUF_RETURNS);
    a.values = B_<float>(c, PPO_BUF_VALUES);
    a.rec_critic = c->rec_critic;
    a.rec_actor = c->rec_actor;
    a.idx = idx;
    a.M = (int)M;
    a.global_M = (double)M * c->world;
    a.inv_global_M = 1.0 / a.global_M;
    c->last_global_M = a.global_M;
    a.adv_stat = c->adv_stats + (size_t)slot * PPO_ADV_PARTS;
    a.adv_norm = c->adv_norm + slot;
    a.slab = c->slab;
    a.stat_slab = c->stat_slab;
    a.stamps = c->stamping ? c->stamps : nullptr;
    a.error_flag = c->error_flag;
    a.single_wave = c->update_single_wave ? 1 : 0;
    bool mfma_now = c->use_mfma;
    if (mfma_now) {   // fp16 range of the matrix-core kernels' operands: see refresh_weight_range
        const ppo_status rs = refresh_weight_range(c);
        if (rs != PPO_OK) return rs;
        if (!c->wr_in_update) wr_snapshot(c);   // a stand-alone step; inside ppo_update the snapshot was taken once, at its start
        if (!weights_fit_update_mfma(c)) { mfma_now = false; c->vector_fallback_launches += 1; }
    }
    if (mfma_now) update_blocks_mfma((int)M, a.n_blocks);
    else a.n_blocks[0] = a.n_blocks[1] = update_blocks_per_net((int)M);
    {
        c->prof_last_sampled = c->prof_every <= 1 || (c->prof_count++ % c->prof_every) == c->prof_every / 2;
        ProfScope ps(c, PROF_FWD_BWD, c->prof_last_sampled);
        if (mfma_now) HIPCHK(c, launch_minibatch_fwd_bwd_mfma(a, c->stream));
        else HIPCHK(c, launch_minibatch_fwd_bwd(a, c->stream));
    }
    c->last_n_blocks[0] = a.n_blocks[0]; c->last_n_blocks[1] = a.n_blocks[1];
    if (reduce) {
        ProfScope ps(c, PROF_REDUCE);
        HIPCHK(c, launch_reduce_grads(c->slab, c->stat_slab, a.n_blocks, c->L, B_<float>(c, PPO_BUF_GRADS), c->loss_sums, c->stream));
    }
    return PPO_OK;
}

// clip + AdamW (or, with do_step false, just the loss scalars and the gradient norm) on whichever parameter layout the context has
static hipError_t clip_adamw_any(ppo_ctx* c, int slot, double global_M, int world, bool do_step, double* clipfrac_accum) {
    if (c->gen && c->gen_opt_fused_ok) {
        if (do_step) c->gen_opt_fused_ok = false;   // its partial sums belong to the gradient the step consumes
        return gen_opt_fused(*c->gen, B_<float>(c, PPO_BUF_PARAMS), B_<float>(c, PPO_BUF_GRADS), B_<float>(c, PPO_BUF_EXP_AVG), B_<float>(c, PPO_BUF_EXP_AVG_SQ),
                             c->cfg.max_grad_norm, c->adam_coefs + slot, c->loss_sums, global_M, c->hp, do_step, c->step_stats + slot, clipfrac_accum, c->error_flag, c->stream);
    }
    if (c->gen) {
        if (do_step) c->gen->planes_dirty = true;
        return gen_clip_adamw(B_<float>(c, PPO_BUF_PARAMS), B_<float>(c, PPO_BUF_GRADS), B_<float>(c, PPO_BUF_EXP_AVG), B_<float>(c, PPO_BUF_EXP_AVG_SQ),
                              c->gen->L, c->cfg.max_grad_norm, c->adam_coefs + slot, c->loss_sums, global_M, c->hp, world, do_step,
                              c->step_stats + slot, clipfrac_accum, c->norm2, c->error_flag, c->stream);
    }
    return launch_clip_adamw(B_<float>(c, PPO_BUF_PARAMS), B_<float>(c, PPO_BUF_GRADS), B_<float>(c, PPO_BUF_EXP_AVG), B_<float>(c, PPO_BUF_EXP_AVG_SQ),
                             c->L, c->cfg.max_grad_norm, c->adam_coefs + slot, c->loss_sums, global_M, c->hp, world, do_step,
                             c->step_stats + slot, clipfrac_accum, c->norm2, c->stream, opt_guard(c));
}

extern "C" ppo_status ppo_minibatch_forward_backward(ppo_ctx* c, const int32_t* idx, int64_t M) {
    NEED(c, c && idx, "null argument");
    DeviceGuard dev_guard(c);
    NEED(c, M >= 1 && M <= c->B, "minibatch size out of range");
    const int slot = c->steps_per_update;  // scratch slot
    {   // stand-alone call: the caller may have rewritten any rollout buffer since the last pack
        if (c->use_mfma && !c->gen) {
            const ppo_status rs = refresh_weight_range(c);
            if (rs != PPO_OK) return rs;
            if (!c->wr_in_update) wr_snapshot(c);
        }
        const ppo_status ps = pack_records(c);
        if (ps != PPO_OK) return ps;
    }
    if (c->cfg.norm_adv) {
        HIPCHK(c, launch_adv_stats(B_<float>(c, PPO_BUF_ADVANTAGES), idx, M, M, 1, c->adv_stats + (size_t)slot * PPO_ADV_PARTS, c->stream));
        ppo_status s = allreduce_sum(c, c->adv_stats + (size_t)slot * PPO_ADV_PARTS, 2 * PPO_ADV_PARTS, true);
        if (s != PPO_OK) return s;
        HIPCHK(c, launch_adv_norm(c->adv_stats + (size_t)slot * PPO_ADV_PARTS, 1, 1, c->B, c->MB, M, c->world, c->adv_norm + slot, c->stream));
    }
    ppo_status s = fwd_bwd(c, idx, M, slot);
    if (s != PPO_OK) return s;
    // loss scalars and the norm of the unclipped gradient, without touching parameters
    HIPCHK(c, clip_adamw_any(c, slot, (double)M * c->world, 1, false, nullptr));
    c->last_stat_slot = slot;
    return PPO_OK;
}

extern "C" ppo_status ppo_allreduce_grads(ppo_ctx* c) {
    NEED(c, c != nullptr, "null ctx");
    DeviceGuard dev_guard(c);
    if (c->world <= 1 && !c->force_collectives) return PPO_OK;
    // the slab reduction already left float copies of the loss sums behind the gradient: one collective carries both
    return allreduce_sum(c, c->buf[PPO_BUF_GRADS], (size_t)c->L.P + 8, false);
}

static ppo_status optimizer_step_slot(ppo_ctx* c, int slot, double global_M, bool coef_on_device) {
    c->opt_step += 1;
    if (!coef_on_device) {
        c->adam_coefs_h[slot] = adam_coef(c->lr, c->opt_step);
        HIPCHK(c, hipMemcpyAsync(c->adam_coefs + slot, c->adam_coefs_h + slot, sizeof(AdamCoef), hipMemcpyHostToDevice, c->stream));
    }
    {
        ProfScope ps(c, PROF_OPT);
        HIPCHK(c, clip_adamw_any(c, slot, global_M, c->force_collectives ? 2 : c->world /* self-test: read the loss sums from the all-reduced tail */, true,
                                 c->clipfrac_accum));
    }
    c->last_stat_slot = slot;
    return PPO_OK;
}

extern "C" ppo_status ppo_optimizer_step(ppo_ctx* c) {
    NEED(c, c != nullptr, "null ctx");
    DeviceGuard dev_guard(c);
    // stand-alone use: the slot's pinned coefficient must not be rewritten while a previous copy is in flight
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // the coefficient is formed from the APPLIED step count: an update that stopped at its target KL enqueued more steps than it applied
    const ppo_status rs = es_resolve(c);
    if (rs != PPO_OK) return rs;
    const ppo_status s = optimizer_step_slot(c, c->steps_per_update, c->last_global_M, false);
    return s != PPO_OK ? s : sweep_weight_range(c, c->stream);
}

extern "C" ppo_status ppo_set_learning_rate(ppo_ctx* c, double lr) {
    NEED(c, c != nullptr, "null ctx");
    c->lr = lr;
    return PPO_OK;
}

// Early stop at a target KL: the host's view of the last update that ran with a target.  Waits for that update's epilogue only (one event behind one
// small copy), never for work enqueued behind it.
static ppo_status es_resolve(ppo_ctx* c) {
    if (!c->es_pending) return PPO_OK;
    DeviceGuard dev_guard(c);
    HIPCHK(c, hipEventSynchronize(c->es_ev));
    c->es_pending = false;
    c->es_last = *c->es_host;
    c->opt_step -= c->es_nominal - c->es_last.applied_total;   // (stand-alone steps taken since stay counted)
    c->epochs_total -= c->es_E - c->es_last.epochs_run;
    return PPO_OK;
}

extern "C" ppo_status ppo_target_kl_set(ppo_ctx* c, double target_kl) {
    NEED(c, c != nullptr, "null ctx");
    if (!std::isfinite(target_kl) || target_kl < 0.0) return fail(c, PPO_ERR_INVALID, "target_kl must be finite and >= 0 (0 = off), got %g", target_kl);
    if (target_kl > 0.0 && !c->es_dev) {
        DeviceGuard dev_guard(c);
        if (!c->es_host) HIPCHK(c, hipHostMalloc(reinterpret_cast<void**>(&c->es_host), sizeof(EarlyStopHost)));
        std::memset(c->es_host, 0, sizeof(EarlyStopHost));
        if (!c->es_ev) HIPCHK(c, hipEventCreateWithFlags(&c->es_ev, hipEventDisableTiming));
        HIPCHK(c, dalloc(c, &c->es_dev, 1));   // last: the launches ask for this one
    }
    c->target_kl = target_kl;
    return PPO_OK;
}

extern "C" ppo_status ppo_target_kl_get(ppo_ctx* c, double* out) {
    NEED(c, c && out, "null argument");
    *out = c->target_kl;
    return PPO_OK;
}

extern "C" ppo_status ppo_early_stop_read(ppo_ctx* c, int32_t* epochs_run, int32_t* stopped, double* kl_at_stop, int64_t* epochs_total) {
    NEED(c, c != nullptr, "null ctx");
    const ppo_status s = es_resolve(c);
    if (s != PPO_OK) return s;
    const bool any = c->updates > 0;
    if (epochs_run) *epochs_run = !any ? 0 : (c->es_last_on ? c->es_last.epochs_run : c->cfg.update_epochs);
    if (stopped) *stopped = any && c->es_last_on ? c->es_last.stopped : 0;
    if (kl_at_stop) *kl_at_stop = any && c->es_last_on ? c->es_last.kl_at_stop : 0.0;
    if (epochs_total) *epochs_total = c->epochs_total;
    return PPO_OK;
}

// All epochs x minibatches of one update, PPO_Discrete.cpp:567-644, then explained variance (:647-648).
extern "C" ppo_status ppo_update(ppo_ctx* c) {
    NEED(c, c != nullptr, "null ctx");
    DeviceGuard dev_guard(c);
    const int E = c->cfg.update_epochs, nmb = c->n_mb;
    ppo_status s = PPO_OK;
    const int32_t* perm = B_<int32_t>(c, PPO_BUF_PERM);
    // returns, values and advantages are fixed for the whole update: the sample records and the explained-variance sums (:647-648) are formed first,
    // so that a sharded run can send its statistics along with the advantage sums
    if (!c->gen) {   // the fp16-range snapshot of this update first: pack_records asks it whether the matrix-core kernel will read the records
        s = refresh_weight_range(c);
        if (s == PPO_OK) s = sweep_weight_range(c, c->wr_stream);
        if (s != PPO_OK) return s;
        wr_snapshot(c);
    }
    // the record pack and the permutations / advantage sums need only the scan's output: ONE launch where the update would launch both, and in a context
    // that is not sharded its last workgroup also carries the normalisations (PPO_KERNEL_SEPARATE_LAUNCHES: the three stand-alone launches)
    const bool sharded = (c->world > 1 || c->force_collectives) && c->world <= 8;
    const bool paired = c->use_mfma && !c->gen && c->cfg.norm_adv && !c->separate_launches;
    const bool norm_folded = paired && c->world == 1 && !c->force_collectives;
    s = pack_records(c, paired, norm_folded);
    if (s != PPO_OK) return s;
    struct InUpdate {
        ppo_ctx* c;
        explicit InUpdate(ppo_ctx* x) : c(x) { c->wr_in_update = true; c->gen_obs_bf_valid = false; }
        ~InUpdate() { c->wr_in_update = false; c->gen_obs_bf_valid = false; }
    } in_update(c);
    if (!c->use_mfma || c->gen)   // otherwise pack_records left the sums
        HIPCHK(c, launch_explained_variance(B_<float>(c, PPO_BUF_RETURNS), B_<float>(c, PPO_BUF_VALUES), c->B, c->ev_sums, c->stream));
    // sharded: this rank's slot of the job-global statistics block (explained-variance sums, its ring of finished episodes with their positions in
    // the reference's push order) rides in front of the advantage sums -- one all-reduce per update, and ppo_read_stats is the same on every rank
    if (sharded) {
        s = consume_finished_episodes(c);
        if (s != PPO_OK) return s;
        HIPCHK(c, launch_gstats_pack(c->ev_sums, c->ring, c->rank, c->gstats, c->stream));
    }
    if (c->cfg.norm_adv) {
        // the advantages and the permutations are fixed for the whole update: the permutations of all epochs and the statistics of ALL
        // minibatches in one launch (and, when sharded, one small all-reduce) instead of a reduction inside every optimizer step
        if (!paired)
            HIPCHK(c, launch_permutations_adv_stats(B_<float>(c, PPO_BUF_ADVANTAGES), B_<int32_t>(c, PPO_BUF_PERM), c->B, E, c->MB, c->cfg.seed, c->updates,
                                                    c->rank, c->adv_stats, c->stream));
        if (sharded) s = allreduce_sum(c, c->gstats, (size_t)PPO_GSTAT_DOUBLES + (size_t)2 * E * nmb * PPO_ADV_PARTS, true);
        else s = allreduce_sum(c, c->adv_stats, (size_t)2 * E * nmb * PPO_ADV_PARTS, true);
        if (s != PPO_OK) return s;
        if (!norm_folded) HIPCHK(c, launch_adv_norm(c->adv_stats, E * nmb, nmb, c->B, c->MB, 0, c->world, c->adv_norm, c->stream, c->clipfrac_accum));   // also: m_clipfracs reset, :564
    } else {
        s = ppo_generate_permutations(c);
        if (s != PPO_OK) return s;
        if (sharded) {
            s = allreduce_sum(c, c->gstats, (size_t)PPO_GSTAT_DOUBLES, true);
            if (s != PPO_OK) return s;
        }
    }
    c->have_gstats = sharded;
    // AdamW scalars of every step of this update, one async copy.  The pinned mirror has two halves used alternately; a half is
    // rewritten only once its previous copy has completed (normally long ago: no stall, and no stream-wide synchronisation).
    {
        const int half = c->coef_half;
        c->coef_half ^= 1;
        AdamCoef* h = c->adam_coefs_h + (size_t)half * (c->steps_per_update + 1);
        HIPCHK(c, hipEventSynchronize(c->coef_copied[half]));
        // the table starts at the APPLIED step count: an update that stopped at its target KL applied fewer steps than it enqueued (es_resolve waits for
        // that update's epilogue, nothing behind it; no-op unless such an update is unresolved)
        s = es_resolve(c);
        if (s != PPO_OK) return s;
        for (int k = 0; k < E * nmb; k++) h[k] = adam_coef(c->lr, c->opt_step + 1 + k);
        HIPCHK(c, hipMemcpyAsync(c->adam_coefs, h, (size_t)E * nmb * sizeof(AdamCoef), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipEventRecord(c->coef_copied[half], c->stream));
    }
    if (!c->cfg.norm_adv) HIPCHK(c, hipMemsetAsync(c->clipfrac_accum, 0, 2 * sizeof(double), c->stream));  // m_clipfracs reset, :564 (with norm_adv: cleared by the adv_norm launch above)
    c->gen_pre_idx = nullptr;   // nothing gathered ahead survives an update (an error return may have left a claim behind)
    // early stop at a target KL: one small launch behind the optimizer launch of every epoch's last minibatch, one behind the update (kernels_earlystop.hip);
    // with no target set, none
    const bool gated = c->target_kl > 0.0;
    const int64_t applied_before = c->opt_step;
    // an update that returns early with an error must not leave a raised stop behind: the epilogue is enqueued on every way out.  The step and epoch
    // counts are undefined after such a failed update (include/ppo_hip.h): nobody knows how much of it was enqueued.
    struct StopScope {
        ppo_ctx* c; bool armed; int E, nmb; int64_t before;
        ~StopScope() {
            if (armed && c->last_stat_slot >= 0)
                (void)launch_kl_gate_end(c->step_stats + c->last_stat_slot, c->clipfrac_accum, c->error_flag, c->es_dev, E, nmb, before, c->stream);
        }
    } stop_scope{ c, false, E, nmb, applied_before };
    auto kl_gate = [&](int e, int mbi, int slot) -> ppo_status {
        if (!gated || mbi != nmb - 1) return PPO_OK;
        HIPCHK(c, launch_kl_gate(c->step_stats + slot, c->target_kl, e, c->clipfrac_accum, c->error_flag, c->es_dev, c->stream));
        stop_scope.armed = true;
        return PPO_OK;
    };
    int k = 0;
    for (int e = 0; e < E; e++) {
        for (int mbi = 0; mbi < nmb; mbi++, k++) {
            const int64_t start = (int64_t)mbi * c->MB;
            const int64_t M = std::min<int64_t>(c->MB, c->B - start);
            const bool fused = c->world == 1 && !c->force_collectives && !c->gen;
            // sharded on the direct-exchange transport: the same two launches, the exchange folded into the slab reduction
            const bool fused_x = c->world > 1 && c->xchg && !c->force_collectives && !c->gen;
            {   // the step after this one (next minibatch, or the first one of the next epoch), for the generic path's gather-ahead
                const bool more = mbi + 1 < nmb || e + 1 < E;
                const int e2 = mbi + 1 < nmb ? e : e + 1, m2 = mbi + 1 < nmb ? mbi + 1 : 0;
                const int64_t start2 = (int64_t)m2 * c->MB;
                c->gen_next_idx = more ? perm + (size_t)e2 * c->B + start2 : nullptr;
                c->gen_next_M = more ? std::min<int64_t>(c->MB, c->B - start2) : 0;
            }
            s = fwd_bwd(c, perm + (size_t)e * c->B + start, M, k, !(fused || fused_x));
            c->gen_next_idx = nullptr;
            if (s != PPO_OK) return s;
            if (fused_x) {
                ExchangeComm& x = *c->xchg;
                c->opt_step += 1;
                x.seq += 1;
                ProfScope ps(c, PROF_OPT);
                HIPCHK(c, launch_reduce_exchange_clip_adamw(c->slab, c->stat_slab, c->last_n_blocks, c->L, B_<float>(c, PPO_BUF_GRADS), c->loss_sums,
                                                            B_<float>(c, PPO_BUF_PARAMS), B_<float>(c, PPO_BUF_EXP_AVG), B_<float>(c, PPO_BUF_EXP_AVG_SQ),
                                                            c->cfg.max_grad_norm, c->adam_coefs + k, (double)M * c->world, c->hp, c->step_stats + k,
                                                            c->clipfrac_accum, c->fused_partial, x.peer, c->rank, c->world, x.slot_bytes, x.seq, x.timeout_flag,
                                                            c->stream, opt_guard(c)));
                c->last_stat_slot = k;
                s = kl_gate(e, mbi, k);
                if (s != PPO_OK) return s;
                continue;
            }
            if (fused) {
                // single rank: two launches (slab reduction + sums of squares, then norm + clip + AdamW) instead of three
                c->opt_step += 1;
                ProfScope ps(c, PROF_OPT);
                HIPCHK(c, launch_reduce_clip_adamw(c->slab, c->stat_slab, c->last_n_blocks, c->L, B_<float>(c, PPO_BUF_GRADS), c->loss_sums, B_<float>(c, PPO_BUF_PARAMS),
                                                   B_<float>(c, PPO_BUF_EXP_AVG), B_<float>(c, PPO_BUF_EXP_AVG_SQ), c->cfg.max_grad_norm, c->adam_coefs + k, (double)M,
                                                   c->hp, c->step_stats + k, c->clipfrac_accum, c->fused_partial, c->stream, opt_guard(c)));
                c->last_stat_slot = k;
                s = kl_gate(e, mbi, k);
                if (s != PPO_OK) return s;
                continue;
            }
            s = ppo_allreduce_grads(c);
            if (s != PPO_OK) return s;
            s = optimizer_step_slot(c, k, (double)M * c->world, true);
            if (s != PPO_OK) return s;
            s = kl_gate(e, mbi, k);
            if (s != PPO_OK) return s;
        }
    }
    c->es_last_on = gated;
    c->epochs_total += E;
    if (gated) {
        stop_scope.armed = false;
        HIPCHK(c, launch_kl_gate_end(c->step_stats + c->last_stat_slot, c->clipfrac_accum, c->error_flag, c->es_dev, E, nmb, applied_before, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->es_host, c->es_dev, sizeof(EarlyStopHost), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipEventRecord(c->es_ev, c->stream));
        c->es_pending = true;
        c->es_nominal = c->opt_step;
        c->es_E = E;
    }
    c->have_ev = true;
    c->updates += 1;
    return PPO_OK;
}

// One iteration of PPO_Discrete::train()'s loop (:511-659) without printing / checkpointing.
// frac = 1.0 - (update - 1.0) / num_updates; lr_now = frac * m_learning_rate  (:515-517), update is 1-based
static void anneal_lr(ppo_ctx* c) {
    if (c->cfg.anneal_lr && c->num_updates_total > 0) {
        const double frac = 1.0 - ((double)(c->updates + 1) - 1.0) / (double)c->num_updates_total;
        c->lr = frac * c->cfg.learning_rate;
    }
}

extern "C" ppo_status ppo_train_iteration(ppo_ctx* c) {
    NEED(c, c != nullptr, "null ctx");
    if (c->host_env) return host_env_refuses(c, "ppo_train_iteration");
    DeviceGuard dev_guard(c);
    anneal_lr(c);
    ppo_status s = ppo_rollout(c, nullptr);
    if (s != PPO_OK) return s;
    // NEXT_VALUE was produced by the rollout's epilogue with the same parameters: go straight to the scan
    s = run_scan(c);
    if (s != PPO_OK) return s;
    return ppo_update(c);
}

// ---------------------------------------------------------------------------------------------------------
// Caller-stepped environments (PPO_ENV_HOST): the rollout of PPO_Discrete::train (:524-548) with the caller's envs stepped between the launches.
// One step path (act_slice / act_slice_f32) with three feeds: the host feed (ppo_host_act commits what ppo_host_observe staged for step t - 1 and acts on
// step t in one launch; the host waits for that launch only, to read the actions), env groups (the same, a group's rows at a time) and the device feed
// (ppo_dev_*).  ppo_host_rollout_end commits step T - 1 and runs the rest of ppo_train_iteration.
// ---------------------------------------------------------------------------------------------------------
static ppo_status host_state(ppo_ctx* c, const char* what) {
    if (!c->host_env)
        return fail(c, PPO_ERR_STATE, "%s: this context steps its own device environment (env_kind %d%s); the ppo_host_* calls serve PPO_ENV_HOST contexts", what,
                    c->cfg.env_kind, env_generic_note(c));
    return PPO_OK;
}

// the staged step and the rollout rows it lands in; t = the step about to be acted on (T at the end of the rollout)
// row0 (env groups): every pointer names row row0 of its array, so that a launch over the group's n_g rows indexes them 0 .. n_g - 1
static HostStepArgs host_args(ppo_ctx* c, int t, bool act_stores, size_t row0, bool staged, bool fin_given) {
    const size_t N = (size_t)c->N;
    const unsigned char* st = c->host_stage_dev;
    const HostStage l = host_stage_layout(c);
    HostStepArgs h{};
    h.st_obs = reinterpret_cast<const float*>(st + l.obs) + row0 * c->O;
    h.st_rew = reinterpret_cast<const float*>(st + l.rew) + row0;
    h.st_done = reinterpret_cast<const int32_t*>(st + l.done) + row0;
    h.st_fin_len = reinterpret_cast<const int32_t*>(st + l.fin_len) + row0;
    h.st_fin_rew = reinterpret_cast<const float*>(st + l.fin_rew) + row0;
    h.commit = staged ? 1 : 0;
    h.fin_given = fin_given ? 1 : 0;
    const size_t prev = (t > 0 ? (size_t)(t - 1) * N : 0) + row0;
    h.rewards_prev = B_<float>(c, PPO_BUF_REWARDS) + prev;
    h.fin_len_prev = B_<int32_t>(c, PPO_BUF_FIN_LEN) + prev;
    h.fin_rew_prev = B_<float>(c, PPO_BUF_FIN_REW) + prev;
    h.next_done = B_<int32_t>(c, PPO_BUF_NEXT_DONE) + row0;
    h.next_obs = B_<float>(c, PPO_BUF_NEXT_OBS) + row0 * c->O;
    h.ep_len = B_<int32_t>(c, PPO_BUF_EP_LEN) + row0;
    h.ep_rew = B_<float>(c, PPO_BUF_EP_REW) + row0;
    if (act_stores) {
        const size_t tn = (size_t)t * N + row0;
        h.obs_t = B_<float>(c, PPO_BUF_OBS) + tn * c->O;
        h.dones_t = B_<float>(c, PPO_BUF_DONES) + tn;
        h.masks_t = c->cfg.dist_kind == PPO_DIST_MASKED ? B_<uint8_t>(c, PPO_BUF_MASKS) + tn * c->A : nullptr;
        h.actions_t = B_<int32_t>(c, PPO_BUF_ACTIONS) + tn * c->H;
    }
    return h;
}
// stepEnvs' outputs (:413-483) for env rows row0 .. row0 + rows, copied into the staging block for the next launch (host memory only: no launch)
static void stage_rows(ppo_ctx* c, size_t row0, size_t rows, const float* next_obs_h, const float* reward_h, const int32_t* done_h, const int32_t* fin_len_h,
                       const float* fin_rew_h) {
    const HostStage l = host_stage_layout(c);
    unsigned char* st = c->host_stage;
    std::memcpy(st + l.obs + row0 * c->O * 4, next_obs_h, rows * c->O * 4);
    std::memcpy(st + l.rew + row0 * 4, reward_h, rows * 4);
    std::memcpy(st + l.done + row0 * 4, done_h, rows * 4);
    if (fin_len_h) {
        std::memcpy(st + l.fin_len + row0 * 4, fin_len_h, rows * 4);
        std::memcpy(st + l.fin_rew + row0 * 4, fin_rew_h, rows * 4);
    }
}
// a host feed's mask rows for the step about to be acted on, copied into the staging block; returns the device's address of the copy, or null when the
// policy is not masked or the caller passed none
static const uint8_t* stage_mask(ppo_ctx* c, size_t row0, size_t rows, const uint8_t* mask_h) {
    if (c->cfg.dist_kind != PPO_DIST_MASKED || mask_h == nullptr) return nullptr;
    const size_t at = host_stage_layout(c).mask + row0 * c->A;
    std::memcpy(c->host_stage + at, mask_h, rows * c->A);
    return c->host_stage_dev + at;
}

// ---- observation normalisation (ppo_obs_norm_*; kernels_obsnorm.hip).  Every batch of new observations -- the reset observations, then each step's
// next_obs -- goes through on_batch in front of the launch that commits it: mode 1 merges the batch into the running statistics and normalises it with
// the merged statistics in one launch, mode 2 normalises with the statistics as they stand.  Everything downstream reads the normalised rows only.
static ppo_status on_reserve(ppo_ctx* c) {
    if (c->on_stats) return PPO_OK;
    DeviceGuard dev_guard(c);
    const size_t O = (size_t)c->O, NO = (size_t)c->N * O;
    std::vector<double> init(2 * O, 0.0);
    for (size_t o = 0; o < O; o++) init[O + o] = 1.0;
    double* st = nullptr;
    HIPCHK(c, dalloc(c, &st, 2 * O, false));
    HIPCHK(c, dalloc(c, &c->on_obs, NO, true));
    HIPCHK(c, dalloc(c, &c->on_final, NO, true));
    HIPCHK(c, hipMemcpy(st, init.data(), 2 * O * sizeof(double), hipMemcpyHostToDevice));
    c->on_stats = st;
    return PPO_OK;
}
// one batch [n, O]: src -> dst (dst may be src) on the context's stream
static ppo_status on_batch(ppo_ctx* c, const float* src, float* dst, int64_t n) {
    if (c->on_mode == 1) {
        HIPCHK(c, launch_obsnorm_update_apply(src, dst, n, c->O, c->on_stats, c->on_count, c->on_eps, c->on_clip, c->stream));
        c->on_count += (double)n;
    } else {
        HIPCHK(c, launch_obsnorm_apply(src, dst, n, c->O, c->on_stats, c->on_eps, c->on_clip, nullptr, nullptr, c->stream));
    }
    return PPO_OK;
}
// the staged step's observations (host-fed rollouts: pinned staging) normalised into the context's scratch, and the commit pointed at the scratch
static ppo_status on_staged(ppo_ctx* c, HostStepArgs& h) {
    if (c->on_mode == 0 || !h.commit) return PPO_OK;
    const ppo_status s = on_batch(c, h.st_obs, c->on_obs, c->N);
    if (s != PPO_OK) return s;
    h.st_obs = c->on_obs;
    return PPO_OK;
}

// ---- reward normalisation (ppo_reward_norm_*; kernels_rewnorm.hip).  Every step's rewards go through rn_batch in front of the launch that commits
// them: mode 1 advances the discounted-return accumulators, merges the N returns into the running statistics and divides the rewards by the merged
// standard deviation in one launch, mode 2 divides by the statistics as they stand.  The commit stores the scratch in the reward row and still sums the
// raw reward into the episode totals.
static ppo_status rn_reserve(ppo_ctx* c) {
    if (c->rn_stats) return PPO_OK;
    DeviceGuard dev_guard(c);
    const double init[2] = {0.0, 1.0};
    double* st = nullptr;
    HIPCHK(c, dalloc(c, &c->rn_ret, (size_t)c->N, true));
    HIPCHK(c, dalloc(c, &c->rn_rew, (size_t)c->N, true));
    HIPCHK(c, dalloc(c, &st, 2, false));
    HIPCHK(c, hipMemcpy(st, init, sizeof(init), hipMemcpyHostToDevice));
    c->rn_stats = st;
    return PPO_OK;
}
// one step: the staged rewards / dones h names -> the context's scratch on the context's stream, and the commit told to store the scratch
static ppo_status rn_batch(ppo_ctx* c, HostStepArgs& h) {
    if (c->rn_mode == 0 || !h.commit) return PPO_OK;
    if (c->rn_mode == 1) {
        HIPCHK(c, launch_rewnorm_update_apply(h.st_rew, h.st_done, c->rn_rew, c->N, c->rn_ret, c->rn_stats, c->rn_count, c->cfg.gamma, c->rn_eps, c->rn_clip,
                                              c->stream));
        c->rn_count += (double)c->N;
    } else {
        HIPCHK(c, launch_rewnorm_apply(h.st_rew, c->rn_rew, c->N, c->rn_stats, c->rn_eps, c->rn_clip, c->stream));
    }
    h.st_rew_store = c->rn_rew;
    return PPO_OK;
}
// Both resets start every env's episode anew: NEXT_DONE = 0, the per-env episode sums = 0, the return accumulators = 0 (reward normalisation: the statistics stay)
static ppo_status reset_episode_state(ppo_ctx* c) {
    HIPCHK(c, hipMemsetAsync(c->buf[PPO_BUF_NEXT_DONE], 0, (size_t)c->N * sizeof(int32_t), c->stream));
    HIPCHK(c, hipMemsetAsync(c->buf[PPO_BUF_EP_LEN], 0, (size_t)c->N * sizeof(int32_t), c->stream));
    HIPCHK(c, hipMemsetAsync(c->buf[PPO_BUF_EP_REW], 0, (size_t)c->N * sizeof(float), c->stream));
    if (c->rn_ret) HIPCHK(c, hipMemsetAsync(c->rn_ret, 0, (size_t)c->N * sizeof(double), c->stream));
    return PPO_OK;
}

// ---- the step, enqueued once for every feed.  A slice is rows row0 .. row0 + rows of step t: the whole batch for ppo_host_act* and ppo_dev_act*, a group's
// rows for ppo_host_group_act.  commit / fin_given: the slice's step t - 1 is staged and not committed yet (never in a device-fed act: ppo_dev_observe
// committed it).  Step t of :524-548: the normalisers over the staged step, its commit, m_obs[t], m_dones[t], the actor forward + sample, m_actions[t],
// m_logprobs[t] (and masks [t]).  action_dev: a device-fed caller's own array; null for a host feed, whose actions go to rows row0 .. of the pinned block.
// The entry points keep their checks, the caller's wait and the state behind the enqueue.
struct StepSlice { int t; size_t row0; int rows; bool commit, fin_given; };
static ppo_status act_slice(ppo_ctx* c, const StepSlice& sl, const uint8_t* mask, int64_t* action_dev) {
    const int N = c->N, n = sl.rows;
    const size_t b = sl.row0, tn = (size_t)sl.t * N + b;
    HostStepArgs h = host_args(c, sl.t, true, b, sl.commit, sl.fin_given);
    // on_staged / rn_batch work on all N rows; groups refuse both normalisers (ppo_host_rollout_begin_groups), so a normaliser implies the whole batch
    NEED(c, (c->on_mode == 0 && c->rn_mode == 0) || (b == 0 && n == N), "a normaliser is on and the step is not the whole batch");
    ppo_status s = on_staged(c, h);   // observation normalisation: one more launch, in front of the commit
    if (s != PPO_OK) return s;
    s = rn_batch(c, h);               // reward normalisation: likewise
    if (s != PPO_OK) return s;
    const int64_t step = c->rollout_steps + sl.t;
    float* logprob_t = B_<float>(c, PPO_BUF_LOGPROBS) + tn;
    if (!c->gen) {   // commit + act in one launch; env_offset + row0 is the sampler's row origin
        HIPCHK(c, launch_host_act(B_<float>(c, PPO_BUF_PARAMS), c->L, c->cfg.dist_kind, mask, n, c->cfg.seed, c->cfg.env_offset + (int64_t)b, step, h,
                                  action_dev ? action_dev : c->host_act_dev + b * c->H, logprob_t, c->host_as16, c->error_flag, c->stream));
        return PPO_OK;
    }
    // generic engine: the commit in place of gen_synthetic_step, then gen_rollout's per-step sequence on the committed observation
    GenericCtx& g = *c->gen;
    int64_t* act64 = action_dev ? action_dev : g.act64 + b * c->H;
    if (h.commit) HIPCHK(c, launch_host_commit(h, n, c->O, c->stream));
    // key_rows = N for every slice.  For a group that is what it always passed.  For the whole batch (n = N, where the callers used to pass 0) it picks
    // the same launch: rows_max = max(MB, N) rounded up to 128 >= N, so the loop in gen_policy is one chunk of rows = N, and its test reads
    // min(rows_max, N) = N <= GEN_FUSED_MAX_ROWS with key_rows = N and rows = N <= GEN_FUSED_MAX_ROWS with key_rows = 0.
    // PPO_KERNEL_CAT_FUSED: the act launch stores the step too
    const CatStepStores stores{ h.next_done, h.obs_t, B_<uint8_t>(c, PPO_BUF_MASKS) + tn * c->A, h.actions_t, logprob_t, h.dones_t };
    bool stored = false;
    s = gen_policy(c, h.next_obs, mask, nullptr, n, step, act64, g.step_lp + b, g.step_en + b, false, (int64_t)b, N, &stores, &stored);
    if (s != PPO_OK) return s;
    if (!stored)
        HIPCHK(c, gen_store_step(g.L, n, h.next_obs, mask, act64, g.step_lp + b, stores.done_prev, stores.obs_t, stores.mask_t, stores.act_t, stores.lp_t, stores.dones_t,
                                 c->stream));
    if (!action_dev) HIPCHK(c, hipMemcpyAsync(c->host_act + b * c->H, act64, (size_t)n * c->H * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    return PPO_OK;
}

// act_slice for a Gaussian context (always the generic engine): the mean in the place of the logits and f32 actions [N,D].  gen_policy_gauss takes no row
// origin and groups refuse Gaussian contexts, so the slice is the whole batch.  action_dev null: the engine's scratch, then one copy into the pinned block.
static ppo_status act_slice_f32(ppo_ctx* c, const StepSlice& sl, float* action_dev) {
    GenericCtx& g = *c->gen;
    const int N = c->N, D = g.L.gauss;
    NEED(c, sl.row0 == 0 && sl.rows == N, "a Gaussian step is not the whole batch");
    HostStepArgs h = host_args(c, sl.t, true, 0, sl.commit, sl.fin_given);
    ppo_status s = on_staged(c, h);
    if (s != PPO_OK) return s;
    s = rn_batch(c, h);
    if (s != PPO_OK) return s;
    if (h.commit) HIPCHK(c, launch_host_commit(h, N, c->O, c->stream));
    float* act = action_dev ? action_dev : g.actf;
    const size_t tn = (size_t)sl.t * N;
    const GaussStepStores stores{ h.next_done, h.obs_t, B_<float>(c, PPO_BUF_ACTIONS) + tn * D, B_<float>(c, PPO_BUF_LOGPROBS) + tn, h.dones_t };
    bool stored = false;
    s = gen_policy_gauss(c, h.next_obs, nullptr, N, c->rollout_steps + sl.t, act, g.step_lp, g.step_en, false, &stores, &stored);
    if (s != PPO_OK) return s;
    if (!stored)
        HIPCHK(c, gen_gauss_store_step(g.L, N, h.next_obs, act, g.step_lp, stores.done_prev, stores.obs_t, stores.act_t, stores.lp_t, stores.dones_t, c->stream));
    if (!action_dev) HIPCHK(c, hipMemcpyAsync(c->host_act, act, (size_t)N * D * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    return PPO_OK;
}

// initEnvs (PPO_Discrete.cpp:365-402) for caller-stepped envs: obs_h f32 [N,O] = every env's reset observation
extern "C" ppo_status ppo_host_env_reset(ppo_ctx* c, const float* obs_h) {
    NEED(c, c != nullptr, "null ctx");
    ppo_status s = host_state(c, "ppo_host_env_reset");
    if (s != PPO_OK) return s;
    if (c->host_phase != 0) return fail(c, PPO_ERR_STATE, "ppo_host_env_reset: a rollout is open (ppo_host_rollout_end first)");
    NEED(c, obs_h != nullptr, "null argument");
    DeviceGuard dev_guard(c);
    s = reset_episode_state(c);
    if (s != PPO_OK) return s;
    HIPCHK(c, hipMemcpyAsync(c->buf[PPO_BUF_NEXT_OBS], obs_h, (size_t)c->N * c->O * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (c->on_mode != 0) {
        s = on_batch(c, B_<float>(c, PPO_BUF_NEXT_OBS), B_<float>(c, PPO_BUF_NEXT_OBS), c->N);
        if (s != PPO_OK) return s;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));   // obs_h is the caller's: consumed before return
    return PPO_OK;
}

// Opens the rollout of one iteration: the LR anneal of ppo_train_iteration (:514-518), the finished episodes of the last rollout into the ring, and the
// choice of arithmetic for the whole rollout from the same weight-range snapshot ppo_rollout takes
static ppo_status host_begin(ppo_ctx* c) {
    DeviceGuard dev_guard(c);
    ppo_status s = consume_finished_episodes(c);
    if (s != PPO_OK) return s;
    bool as16 = false;
    if (!c->gen) {
        as16 = !c->rollout_vector && policy_act16_serves(c->L);
        if (as16) {
            s = refresh_weight_range(c);
            if (s != PPO_OK) return s;
            wr_snapshot(c);
            if (!weights_fit_rollout16(c)) { as16 = false; c->vector_fallback_launches += 1; }
        }
    }
    anneal_lr(c);
    c->host_as16 = as16;
    c->host_phase = 1;
    c->host_t = 0;
    c->host_staged = false;
    c->host_fin_given = false;
    c->host_n_groups = 0;
    c->host_feed = 0;
    return PPO_OK;
}
extern "C" ppo_status ppo_host_rollout_begin(ppo_ctx* c) {
    NEED(c, c != nullptr, "null ctx");
    ppo_status s = host_state(c, "ppo_host_rollout_begin");
    if (s != PPO_OK) return s;
    if (c->host_n_groups > 0) return fail(c, PPO_ERR_STATE, "ppo_host_rollout_begin: a rollout of %d env groups is already open", c->host_n_groups);
    if (c->host_phase != 0) return fail(c, PPO_ERR_STATE, "ppo_host_rollout_begin: a rollout is already open (%d of %d steps acted on)", c->host_t, c->T);
    return host_begin(c);
}

// how a host-fed act ends: the one wait of a step, the actions into the caller's array, and the state behind the enqueue
static ppo_status host_acted(ppo_ctx* c, void* action_h, size_t bytes) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::memcpy(action_h, c->host_act, bytes);
    c->host_staged = false;
    c->host_t += 1;
    c->host_phase = 2;
    c->host_feed = 1;
    return PPO_OK;
}

// Step t for the whole batch, the mask through the staging block; returns when action_h holds the actions
extern "C" ppo_status ppo_host_act(ppo_ctx* c, const uint8_t* mask_h, int64_t* action_h) {
    NEED(c, c != nullptr, "null ctx");
    ppo_status s = host_state(c, "ppo_host_act");
    if (s != PPO_OK) return s;
    if (is_gauss(c)) return wrong_action_type(c, "ppo_host_act", "ppo_host_act_f32");
    if (c->host_n_groups > 0) return fail(c, PPO_ERR_STATE, "ppo_host_act: the open rollout is taken by env groups (ppo_host_group_act)");
    if (c->host_phase == 0) return fail(c, PPO_ERR_STATE, "ppo_host_act: no rollout is open (ppo_host_rollout_begin)");
    if (c->host_feed == 2)
        return fail(c, PPO_ERR_STATE, "ppo_host_act: the open rollout is device-fed (ppo_dev_act / ppo_dev_observe); a rollout takes the ppo_host_* or the ppo_dev_* calls, not both");
    if (c->host_phase == 2) return fail(c, PPO_ERR_STATE, "ppo_host_act: step %d was acted on and not observed (ppo_host_observe)", c->host_t - 1);
    if (c->host_t >= c->T) return fail(c, PPO_ERR_STATE, "ppo_host_act: all %d steps of the rollout are taken (ppo_host_rollout_end)", c->T);
    NEED(c, action_h != nullptr, "null argument");
    DeviceGuard dev_guard(c);
    const int N = c->N;
    s = act_slice(c, StepSlice{ c->host_t, 0, N, c->host_staged, c->host_fin_given }, stage_mask(c, 0, (size_t)N, mask_h), nullptr);
    if (s != PPO_OK) return s;
    return host_acted(c, action_h, (size_t)N * c->H * sizeof(int64_t));
}

// ppo_host_act for a Gaussian context: f32 actions [N,D]
extern "C" ppo_status ppo_host_act_f32(ppo_ctx* c, float* action_h) {
    NEED(c, c != nullptr, "null ctx");
    ppo_status s = host_state(c, "ppo_host_act_f32");
    if (s != PPO_OK) return s;
    if (!is_gauss(c)) return wrong_action_type(c, "ppo_host_act_f32", "ppo_host_act");
    if (c->host_phase == 0) return fail(c, PPO_ERR_STATE, "ppo_host_act_f32: no rollout is open (ppo_host_rollout_begin)");
    if (c->host_feed == 2)
        return fail(c, PPO_ERR_STATE, "ppo_host_act_f32: the open rollout is device-fed (ppo_dev_act_f32 / ppo_dev_observe); a rollout takes the ppo_host_* or the ppo_dev_* calls, not both");
    if (c->host_phase == 2) return fail(c, PPO_ERR_STATE, "ppo_host_act_f32: step %d was acted on and not observed (ppo_host_observe)", c->host_t - 1);
    if (c->host_t >= c->T) return fail(c, PPO_ERR_STATE, "ppo_host_act_f32: all %d steps of the rollout are taken (ppo_host_rollout_end)", c->T);
    NEED(c, action_h != nullptr, "null argument");
    DeviceGuard dev_guard(c);
    s = act_slice_f32(c, StepSlice{ c->host_t, 0, c->N, c->host_staged, c->host_fin_given }, nullptr);
    if (s != PPO_OK) return s;
    return host_acted(c, action_h, (size_t)c->N * c->gen->L.gauss * sizeof(float));
}

// ---- truncation events: the partial-episode bootstrap for episodes a time limit cut off (the reference ends them like terminal states,
// PPO_Discrete.cpp:443-452).  The observes keep (t * N + n, final observation) on the host; ppo_host_rollout_end folds gamma * V(final obs) into the rewards.
static inline int32_t* trunc_idx_h(ppo_ctx* c) { return reinterpret_cast<int32_t*>(c->trunc_h); }
static inline float* trunc_obs_h(ppo_ctx* c) { return reinterpret_cast<float*>(c->trunc_h + (size_t)c->trunc_cap * 4); }
static inline float* trunc_val_h(ppo_ctx* c) { return reinterpret_cast<float*>(c->trunc_h + (size_t)c->trunc_cap * 4 * (1 + c->O)); }
static inline int32_t* trunc_idx_d(ppo_ctx* c) { return reinterpret_cast<int32_t*>(c->trunc_dev); }
static inline float* trunc_obs_d(ppo_ctx* c) { return reinterpret_cast<float*>(c->trunc_dev + (size_t)c->trunc_cap * 4); }
static inline float* trunc_val_d(ppo_ctx* c) { return reinterpret_cast<float*>(c->trunc_dev + (size_t)c->trunc_cap * 4 * (1 + c->O)); }

// Room for `need` entries: doubling, at most max(T * N, need) (a rollout has at most one event per step and env), the open rollout's events and the
// last closed rollout's values carried over.  The one place these blocks are allocated -- ppo_evaluate's policy (ppo_ctx_create in ppo_hip.h).
static ppo_status trunc_reserve(ppo_ctx* c, int64_t need) {
    if (need <= c->trunc_cap) return PPO_OK;
    int64_t cap = std::max<int64_t>(c->trunc_cap, 64);
    while (cap < need) cap *= 2;
    cap = (std::min<int64_t>(cap, std::max<int64_t>((int64_t)c->T * c->N, need)) + 3) & ~(int64_t)3;   // a multiple of 4: the observation area stays 16-byte aligned
    const size_t bytes = (size_t)cap * 4 * (2 + c->O);
    DeviceGuard dev_guard(c);
    HIPCHK(c, hipStreamSynchronize(c->stream));   // nothing enqueued may still be using the blocks that are replaced
    if (!c->trunc_ev) HIPCHK(c, hipEventCreateWithFlags(&c->trunc_ev, hipEventDisableTiming));
    unsigned char *h = nullptr, *d = nullptr;
    HIPCHK(c, hipHostMalloc(reinterpret_cast<void**>(&h), bytes, hipHostMallocDefault));
    if (hipMalloc(reinterpret_cast<void**>(&d), bytes) != hipSuccess) {
        (void)hipHostFree(h);
        return fail(c, PPO_ERR_HIP, "no device memory for %lld truncation events", (long long)cap);
    }
    if (c->trunc_h) {
        std::memcpy(h, trunc_idx_h(c), (size_t)c->trunc_n * 4);
        std::memcpy(h + (size_t)cap * 4, trunc_obs_h(c), (size_t)c->trunc_n * c->O * 4);
        std::memcpy(h + (size_t)cap * 4 * (1 + c->O), trunc_val_h(c), c->trunc_last_idx.size() * 4);
        (void)hipHostFree(c->trunc_h);
        (void)hipFree(c->trunc_dev);
    }
    c->trunc_h = h; c->trunc_dev = d; c->trunc_cap = cap;
    return PPO_OK;
}

// The checks of a _truncated observe over `rows` rows starting at env row0, then room for its events.  Changes nothing the rollout can see.
static ppo_status trunc_check(ppo_ctx* c, const char* what, const int32_t* done_h, const int32_t* truncated_h, const float* final_obs_h, size_t row0, size_t rows,
                              int64_t* n_events) {
    int64_t k = 0;
    if (truncated_h)
        for (size_t n = 0; n < rows; n++) {
            if (truncated_h[n] == 0) continue;
            if (done_h[n] == 0) return fail(c, PPO_ERR_INVALID, "%s: env row %lld is flagged truncated but not done (a truncation ends the episode)", what, (long long)(row0 + n));
            k++;
        }
    if (k > 0 && final_obs_h == nullptr) return fail(c, PPO_ERR_INVALID, "%s: %lld rows are flagged truncated and final_obs_h is null", what, (long long)k);
    *n_events = k;
    return k > 0 ? trunc_reserve(c, c->trunc_n + k) : PPO_OK;
}
// the events of step t, rows row0 .. row0 + rows, behind the list (room was made by trunc_check)
static void trunc_append(ppo_ctx* c, int t, const int32_t* truncated_h, const float* final_obs_h, size_t row0, size_t rows) {
    if (c->trunc_n == 0 && !c->trunc_last_idx.empty()) (void)hipEventSynchronize(c->trunc_ev);   // the last rollout's copy has read the list (long since: an act was waited for)
    for (size_t n = 0; n < rows; n++) {
        if (truncated_h[n] == 0) continue;
        trunc_idx_h(c)[c->trunc_n] = (int32_t)((size_t)t * c->N + row0 + n);
        std::memcpy(trunc_obs_h(c) + (size_t)c->trunc_n * c->O, final_obs_h + n * c->O, (size_t)c->O * 4);
        c->trunc_n++;
    }
}

// stepEnvs' outputs for step t (:413-483), staged for the next launch (host memory only: no launch)
static ppo_status host_observe_common(ppo_ctx* c, const char* what, const float* next_obs_h, const float* reward_h, const int32_t* done_h, const int32_t* fin_len_h,
                                      const float* fin_rew_h, const int32_t* truncated_h, const float* final_obs_h) {
    NEED(c, c != nullptr, "null ctx");
    ppo_status s = host_state(c, what);
    if (s != PPO_OK) return s;
    if (c->host_n_groups > 0) return fail(c, PPO_ERR_STATE, "%s: the open rollout is taken by env groups (ppo_host_group_observe)", what);
    if (c->host_feed == 2)
        return fail(c, PPO_ERR_STATE, "%s: the open rollout is device-fed (ppo_dev_act / ppo_dev_observe); a rollout takes the ppo_host_* or the ppo_dev_* calls, not both", what);
    if (c->host_phase != 2) return fail(c, PPO_ERR_STATE, "%s: no step awaits its observation (ppo_host_act first)", what);
    NEED(c, next_obs_h && reward_h && done_h, "null argument");
    NEED(c, (fin_len_h == nullptr) == (fin_rew_h == nullptr), "fin_len_h and fin_rew_h: both or neither");
    const size_t N = (size_t)c->N;
    int64_t n_events = 0;
    s = trunc_check(c, what, done_h, truncated_h, final_obs_h, 0, N, &n_events);
    if (s != PPO_OK) return s;
    if (n_events > 0) trunc_append(c, c->host_t - 1, truncated_h, final_obs_h, 0, N);
    stage_rows(c, 0, N, next_obs_h, reward_h, done_h, fin_len_h, fin_rew_h);
    c->host_fin_given = fin_len_h != nullptr;
    c->host_staged = true;
    c->host_phase = 1;
    return PPO_OK;
}
extern "C" ppo_status ppo_host_observe(ppo_ctx* c, const float* next_obs_h, const float* reward_h, const int32_t* done_h, const int32_t* fin_len_h,
                                       const float* fin_rew_h) {
    return host_observe_common(c, "ppo_host_observe", next_obs_h, reward_h, done_h, fin_len_h, fin_rew_h, nullptr, nullptr);
}
extern "C" ppo_status ppo_host_observe_truncated(ppo_ctx* c, const float* next_obs_h, const float* reward_h, const int32_t* done_h, const int32_t* fin_len_h,
                                                 const float* fin_rew_h, const int32_t* truncated_h, const float* final_obs_h) {
    return host_observe_common(c, "ppo_host_observe_truncated", next_obs_h, reward_h, done_h, fin_len_h, fin_rew_h, truncated_h, final_obs_h);
}

// ---- env groups: the same rollout, group by group.  One stream: launches run in the order they were enqueued, and the activation scratch of the generic
// engine (per context) is never used by two groups at once; what is per group is the host's wait (an event behind the group's act) and the place in
// the rollout.  A group's rows of the staging block and of the action block are written by the host / the device only between that group's own calls,
// which its phase keeps in order, so no group waits for another.
static ppo_status host_group_state(ppo_ctx* c, const char* what, int32_t g) {
    ppo_status s = host_state(c, what);
    if (s != PPO_OK) return s;
    if (c->host_n_groups == 0)
        return fail(c, PPO_ERR_STATE, c->host_phase == 0 ? "%s: no rollout is open (ppo_host_rollout_begin_groups)"
                                                         : "%s: the open rollout was not opened with env groups (ppo_host_act / ppo_host_observe)", what);
    if (g < 0 || g >= c->host_n_groups) return fail(c, PPO_ERR_INVALID, "%s: group %d of %d", what, (int)g, c->host_n_groups);
    return PPO_OK;
}

extern "C" ppo_status ppo_host_rollout_begin_groups(ppo_ctx* c, int32_t n_groups, const int32_t* bounds_h) {
    NEED(c, c != nullptr, "null ctx");
    ppo_status s = host_state(c, "ppo_host_rollout_begin_groups");
    if (s != PPO_OK) return s;
    if (c->host_n_groups > 0) return fail(c, PPO_ERR_STATE, "ppo_host_rollout_begin_groups: a rollout of %d env groups is already open", c->host_n_groups);
    if (c->host_phase != 0) return fail(c, PPO_ERR_STATE, "ppo_host_rollout_begin_groups: a rollout is already open (%d of %d steps acted on)", c->host_t, c->T);
    if (c->on_mode != 0)
        return fail(c, PPO_ERR_UNSUPPORTED, "ppo_host_rollout_begin_groups: observation normalisation is on (ppo_obs_norm_enable): groups commit their steps in an "
                                            "order the caller chooses and the running statistics would depend on it, which breaks the groups' promise of "
                                            "interleaving-independent bits; use ppo_host_rollout_begin, or turn the normalisation off");
    if (is_gauss(c))
        return fail(c, PPO_ERR_UNSUPPORTED, "ppo_host_rollout_begin_groups: env groups are not built for PPO_DIST_GAUSSIAN contexts; use ppo_host_rollout_begin");
    if (c->rn_mode != 0)
        return fail(c, PPO_ERR_UNSUPPORTED, "ppo_host_rollout_begin_groups: reward normalisation is on (ppo_reward_norm_enable): groups commit their steps in an "
                                            "order the caller chooses and the running statistics would depend on it, which breaks the groups' promise of "
                                            "interleaving-independent bits; use ppo_host_rollout_begin, or turn the normalisation off");
    NEED(c, bounds_h != nullptr, "null argument");
    if (n_groups < 1 || n_groups > PPO_HOST_MAX_GROUPS)
        return fail(c, PPO_ERR_INVALID, "ppo_host_rollout_begin_groups: n_groups %d outside 1 .. %d", (int)n_groups, PPO_HOST_MAX_GROUPS);
    if (bounds_h[0] != 0 || bounds_h[n_groups] != c->N)
        return fail(c, PPO_ERR_INVALID, "ppo_host_rollout_begin_groups: bounds run from %d to %d, not from 0 to num_envs = %d", (int)bounds_h[0], (int)bounds_h[n_groups], c->N);
    for (int g = 0; g < n_groups; g++)
        if (bounds_h[g + 1] <= bounds_h[g])
            return fail(c, PPO_ERR_INVALID, "ppo_host_rollout_begin_groups: group %d is empty or reversed (rows %d .. %d)", g, (int)bounds_h[g], (int)bounds_h[g + 1]);
    s = host_begin(c);
    if (s != PPO_OK) return s;
    for (int g = 0; g < n_groups; g++) {
        ppo_ctx::HostGroup& G = c->host_grp[g];
        G.row0 = bounds_h[g]; G.rows = bounds_h[g + 1] - bounds_h[g];
        G.t = 0; G.phase = 1; G.staged = false; G.fin_given = false;
    }
    c->host_n_groups = n_groups;
    return PPO_OK;
}

extern "C" ppo_status ppo_host_group_act(ppo_ctx* c, int32_t g, const uint8_t* mask_h) {
    NEED(c, c != nullptr, "null ctx");
    ppo_status s = host_group_state(c, "ppo_host_group_act", g);
    if (s != PPO_OK) return s;
    ppo_ctx::HostGroup& G = c->host_grp[g];
    if (G.phase == 2) return fail(c, PPO_ERR_STATE, "ppo_host_group_act: group %d: the actions of step %d were not read (ppo_host_group_actions)", (int)g, G.t - 1);
    if (G.phase == 3) return fail(c, PPO_ERR_STATE, "ppo_host_group_act: group %d: step %d was acted on and not observed (ppo_host_group_observe)", (int)g, G.t - 1);
    if (G.t >= c->T) return fail(c, PPO_ERR_STATE, "ppo_host_group_act: group %d: all %d steps of the rollout are taken (ppo_host_rollout_end)", (int)g, c->T);
    DeviceGuard dev_guard(c);
    const uint8_t* mask = stage_mask(c, (size_t)G.row0, (size_t)G.rows, mask_h);
    s = act_slice(c, StepSlice{ G.t, (size_t)G.row0, G.rows, G.staged, G.fin_given }, mask, nullptr);
    if (s != PPO_OK) return s;
    HIPCHK(c, hipEventRecord(G.ev, c->stream));
    G.staged = false;
    G.t += 1;
    G.phase = 2;
    return PPO_OK;
}

extern "C" ppo_status ppo_host_group_actions(ppo_ctx* c, int32_t g, int64_t* action_h) {
    NEED(c, c != nullptr, "null ctx");
    ppo_status s = host_group_state(c, "ppo_host_group_actions", g);
    if (s != PPO_OK) return s;
    ppo_ctx::HostGroup& G = c->host_grp[g];
    if (G.phase != 2)
        return fail(c, PPO_ERR_STATE, "ppo_host_group_actions: group %d: no act awaits its read at step %d (%s)", (int)g, G.t,
                    G.phase == 1 ? "ppo_host_group_act first" : "the actions were read; ppo_host_group_observe is next");
    NEED(c, action_h != nullptr, "null argument");
    DeviceGuard dev_guard(c);
    HIPCHK(c, hipEventSynchronize(G.ev));   // this group's act only: what other groups enqueued behind it keeps running
    std::memcpy(action_h, c->host_act + (size_t)G.row0 * c->H, (size_t)G.rows * c->H * sizeof(int64_t));
    G.phase = 3;
    return PPO_OK;
}

static ppo_status host_group_observe_common(ppo_ctx* c, const char* what, int32_t g, const float* next_obs_h, const float* reward_h, const int32_t* done_h,
                                            const int32_t* fin_len_h, const float* fin_rew_h, const int32_t* truncated_h, const float* final_obs_h) {
    NEED(c, c != nullptr, "null ctx");
    ppo_status s = host_group_state(c, what, g);
    if (s != PPO_OK) return s;
    ppo_ctx::HostGroup& G = c->host_grp[g];
    if (G.phase != 3)
        return fail(c, PPO_ERR_STATE, "%s: group %d: no step awaits its observation at step %d (%s)", what, (int)g, G.t,
                    G.phase == 1 ? "ppo_host_group_act first" : "ppo_host_group_actions first");
    NEED(c, next_obs_h && reward_h && done_h, "null argument");
    NEED(c, (fin_len_h == nullptr) == (fin_rew_h == nullptr), "fin_len_h and fin_rew_h: both or neither");
    const size_t b = (size_t)G.row0, n = (size_t)G.rows;
    int64_t n_events = 0;
    s = trunc_check(c, what, done_h, truncated_h, final_obs_h, b, n, &n_events);
    if (s != PPO_OK) return s;
    if (n_events > 0) trunc_append(c, G.t - 1, truncated_h, final_obs_h, b, n);
    stage_rows(c, b, n, next_obs_h, reward_h, done_h, fin_len_h, fin_rew_h);
    G.fin_given = fin_len_h != nullptr;
    G.staged = true;
    G.phase = 1;
    return PPO_OK;
}
extern "C" ppo_status ppo_host_group_observe(ppo_ctx* c, int32_t g, const float* next_obs_h, const float* reward_h, const int32_t* done_h,
                                             const int32_t* fin_len_h, const float* fin_rew_h) {
    return host_group_observe_common(c, "ppo_host_group_observe", g, next_obs_h, reward_h, done_h, fin_len_h, fin_rew_h, nullptr, nullptr);
}
extern "C" ppo_status ppo_host_group_observe_truncated(ppo_ctx* c, int32_t g, const float* next_obs_h, const float* reward_h, const int32_t* done_h,
                                                       const int32_t* fin_len_h, const float* fin_rew_h, const int32_t* truncated_h, const float* final_obs_h) {
    return host_group_observe_common(c, "ppo_host_group_observe_truncated", g, next_obs_h, reward_h, done_h, fin_len_h, fin_rew_h, truncated_h, final_obs_h);
}

// The fold of ppo_bootstrap_rewards with the context's critic, on the path the context's values take (ppo_host_rollout_end, ppo_get_value)
static ppo_status bootstrap_launch(ppo_ctx* c, const float* final_obs, const int32_t* index, int64_t K, float gamma, float* rewards, float* value_out) {
    if (c->gen) {
        const ppo_status s = gen_values(c, final_obs, K, value_out);
        if (s != PPO_OK) return s;
        HIPCHK(c, gen_fold_rewards(value_out, index, K, gamma, rewards, c->stream));
    } else if (critic_is_mfma(c)) {
        HIPCHK(c, launch_bootstrap_values_mfma(B_<float>(c, PPO_BUF_PARAMS), c->L, final_obs, index, K, gamma, rewards, value_out, c->stream));
    } else {
        HIPCHK(c, launch_bootstrap_values(B_<float>(c, PPO_BUF_PARAMS), c->L, final_obs, index, K, gamma, rewards, value_out, c->stream));
    }
    return PPO_OK;
}

extern "C" ppo_status ppo_bootstrap_rewards(ppo_ctx* c, const float* final_obs, const int32_t* index, int64_t K, float gamma, float* rewards, float* value_out) {
    NEED(c, c != nullptr, "null ctx");
    NEED(c, K >= 0, "ppo_bootstrap_rewards: K < 0");
    if (K == 0) return PPO_OK;
    NEED(c, final_obs && index && rewards, "ppo_bootstrap_rewards: null argument");
    DeviceGuard dev_guard(c);
    if (c->gen && !value_out) {   // the generic engine's critic writes its values somewhere: the event block's value area (of the device block; the host's is not touched)
        const ppo_status s = trunc_reserve(c, std::max<int64_t>(K, c->trunc_n));
        if (s != PPO_OK) return s;
        value_out = trunc_val_d(c);
    }
    return bootstrap_launch(c, final_obs, index, K, gamma, rewards, value_out);
}

// ppo_host_rollout_end, behind the value launch and in front of the scan: the open rollout's events, sorted by index so that the outcome does not depend on
// how groups interleaved, in ONE asynchronous copy; the fold on REWARDS; the values back into the host block.  No event: nothing is enqueued.
static ppo_status host_fold_truncations(ppo_ctx* c) {
    const int64_t K = c->trunc_n, cap = c->trunc_cap;
    c->trunc_n = 0;
    if (K == 0) { c->trunc_last_idx.clear(); return PPO_OK; }
    int32_t* ix = trunc_idx_h(c);
    float* ob = trunc_obs_h(c);
    const size_t O = (size_t)c->O;
    if (!std::is_sorted(ix, ix + K)) {
        c->trunc_order.resize((size_t)K);
        for (int64_t k = 0; k < K; k++) c->trunc_order[(size_t)k] = (int32_t)k;
        std::sort(c->trunc_order.begin(), c->trunc_order.end(), [ix](int32_t a, int32_t b) { return ix[a] < ix[b]; });
        c->trunc_sorted.resize((size_t)K * O);
        for (int64_t k = 0; k < K; k++) std::memcpy(c->trunc_sorted.data() + (size_t)k * O, ob + (size_t)c->trunc_order[(size_t)k] * O, O * 4);
        std::memcpy(ob, c->trunc_sorted.data(), (size_t)K * O * 4);
        for (int64_t k = 0; k < K; k++) c->trunc_order[(size_t)k] = ix[c->trunc_order[(size_t)k]];
        std::memcpy(ix, c->trunc_order.data(), (size_t)K * 4);
    }
    c->trunc_last_idx.assign(ix, ix + K);
    // the K indices move to the END of the index area, where the observation area begins: indices and observations are then one contiguous range
    const size_t off = (size_t)(cap - K) * 4;
    std::memmove(c->trunc_h + off, ix, (size_t)K * 4);
    HIPCHK(c, hipMemcpyAsync(c->trunc_dev + off, c->trunc_h + off, (size_t)K * 4 * (1 + O), hipMemcpyHostToDevice, c->stream));
    if (c->on_mode != 0)   // the final observations by the statistics as they stand now (the end of the rollout), without updating them
        HIPCHK(c, launch_obsnorm_apply(trunc_obs_d(c), trunc_obs_d(c), K, c->O, c->on_stats, c->on_eps, c->on_clip, nullptr, nullptr, c->stream));
    const ppo_status s = bootstrap_launch(c, trunc_obs_d(c), trunc_idx_d(c) + (cap - K), K, c->cfg.gamma, B_<float>(c, PPO_BUF_REWARDS), trunc_val_d(c));
    if (s != PPO_OK) return s;
    HIPCHK(c, hipMemcpyAsync(trunc_val_h(c), trunc_val_d(c), (size_t)K * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipEventRecord(c->trunc_ev, c->stream));
    return PPO_OK;
}

// The truncation events of the last closed rollout: flat indices t * N + n ascending and the values V(final obs) that were folded in
extern "C" ppo_status ppo_host_truncations(ppo_ctx* c, int64_t* count, int32_t* index_h, float* value_h, int64_t cap) {
    NEED(c, c != nullptr, "null ctx");
    const ppo_status s = host_state(c, "ppo_host_truncations");
    if (s != PPO_OK) return s;
    NEED(c, count != nullptr, "ppo_host_truncations: count is null");
    if (c->dev_last >= 0)   // the last closed rollout was device-fed and folded: its list is on the device
        return events_read(c, c->dev_events[c->dev_last], "ppo_host_truncations", count, index_h, value_h, cap);
    const int64_t K = (int64_t)c->trunc_last_idx.size();
    if ((index_h || value_h) && cap < K)
        return fail(c, PPO_ERR_INVALID, "ppo_host_truncations: room for %lld events, the last rollout had %lld", (long long)cap, (long long)K);
    if (K > 0 && index_h) std::memcpy(index_h, c->trunc_last_idx.data(), (size_t)K * 4);
    if (K > 0 && value_h) {
        DeviceGuard dev_guard(c);
        HIPCHK(c, hipEventSynchronize(c->trunc_ev));   // the fold and the copy of its values: the update behind them keeps running
        std::memcpy(value_h, trunc_val_h(c), (size_t)K * 4);
    }
    *count = K;
    return PPO_OK;
}

// Time-limit truncations of the context's own device env (ppo_hip.h: ppo_env_truncation_bootstrap).  Which contexts the two calls serve:
static ppo_status envt_state(ppo_ctx* c, const char* what) {
    if (c->host_env)
        return fail(c, PPO_ERR_UNSUPPORTED, "%s: this context's environments are the caller's (PPO_ENV_HOST), and only the caller holds the observation an episode "
                                            "ended on: pass it with ppo_host_observe_truncated (ppo_dev_observe for device arrays)", what);
    if (c->env)   // its observation holds its state and the fold runs on the fused critic (fused_env_fold_truncations), or the row says why not
        return (c->env->folds || c->cut_state) ? PPO_OK
                             : fail(c, PPO_ERR_UNSUPPORTED, "%s: the fold rebuilds the final observation of a cut-off episode from PPO_BUF_OBS, and a %s: not built "
                                                            "for this env", what, c->env->text.no_fold);
    if (c->env_generic)
        return fail(c, PPO_ERR_UNSUPPORTED, "%s: the fold of CartPole / MountainCar is built on the reference-shape critic (2 x 64), and this context's network lives "
                                            "on the generic engine (PPO_KERNEL_ENV_GENERIC): not built for it", what);
    if (c->cfg.env_kind != PPO_ENV_CARTPOLE && c->cfg.env_kind != PPO_ENV_MOUNTAINCAR)
        return fail(c, PPO_ERR_UNSUPPORTED, "%s: the synthetic env's observations are noise: an episode there has no last observation to bootstrap from", what);
    return PPO_OK;
}
extern "C" ppo_status ppo_env_truncation_bootstrap(ppo_ctx* c, int32_t on) {
    NEED(c, c != nullptr, "null ctx");
    const ppo_status s = envt_state(c, "ppo_env_truncation_bootstrap");
    if (s != PPO_OK) return s;
    NEED(c, on == 0 || on == 1, "ppo_env_truncation_bootstrap: on must be 0 or 1");
    if (on) {   // the event list, made by the first enable
        DeviceGuard dev_guard(c);
        const ppo_status r = events_reserve(c, c->env_events, c->B);
        if (r != PPO_OK) return r;
    }
    c->envt_on = on != 0;
    return PPO_OK;
}
// The events of the last ppo_rollout (ppo_host_truncations' contract); none before the first rollout, or when the last one ran with the switch off
extern "C" ppo_status ppo_env_truncations(ppo_ctx* c, int64_t* count, int32_t* index_h, float* value_h, int64_t cap) {
    NEED(c, c != nullptr, "null ctx");
    const ppo_status s = envt_state(c, "ppo_env_truncations");
    if (s != PPO_OK) return s;
    NEED(c, count != nullptr, "ppo_env_truncations: count is null");
    return events_read(c, c->env_events, "ppo_env_truncations", count, index_h, value_h, cap);
}

// ---------------------------------------------------------------------------------------------------------
// Caller-stepped environments on the device (ppo_dev_*): the same rollout fed from DEVICE arrays in stream order (the reference's loop, PPO_Discrete.cpp:365-483,
// 524-548, with the envs on the chip).  Every call only enqueues: no host wait, no host copy of per-step data.  The hand-over between the caller's stream
// and the context's (non-blocking) stream is a pair of events per call; caller_stream == the context's stream needs none.  ppo_dev_act is act_slice
// with commit = 0 on the caller's action array; ppo_dev_observe is host_commit_kernel on the caller's arrays, at once, and -- with flags -- the fold kernel
// that finds the flagged rows itself (launch_dev_fold*; gauss_fused_dev_fold for the two fused families).  ppo_host_rollout_end then has nothing to commit and nothing to fold.
// ---------------------------------------------------------------------------------------------------------
static ppo_status dev_handover_in(ppo_ctx* c, hipStream_t caller) {
    if (caller == c->stream) return PPO_OK;
    if (!c->dev_ev_in) HIPCHK(c, hipEventCreateWithFlags(&c->dev_ev_in, hipEventDisableTiming));
    if (!c->dev_ev_out) HIPCHK(c, hipEventCreateWithFlags(&c->dev_ev_out, hipEventDisableTiming));
    HIPCHK(c, hipEventRecord(c->dev_ev_in, caller));
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->dev_ev_in, 0));
    return PPO_OK;
}
static ppo_status dev_handover_out(ppo_ctx* c, hipStream_t caller) {
    if (caller == c->stream) return PPO_OK;
    HIPCHK(c, hipEventRecord(c->dev_ev_out, c->stream));
    HIPCHK(c, hipStreamWaitEvent(caller, c->dev_ev_out, 0));
    return PPO_OK;
}
// what every ppo_dev_* call of an open rollout checks first
static ppo_status dev_state(ppo_ctx* c, const char* what) {
    ppo_status s = host_state(c, what);
    if (s != PPO_OK) return s;
    if (c->host_n_groups > 0)
        return fail(c, PPO_ERR_STATE, "%s: the open rollout is taken by env groups (ppo_host_group_*); groups hide a host wait that the ppo_dev_* calls do not have", what);
    if (c->host_feed == 1)
        return fail(c, PPO_ERR_STATE, "%s: the open rollout is host-fed (ppo_host_act / ppo_host_observe); a rollout takes the ppo_host_* or the ppo_dev_* calls, not both", what);
    return PPO_OK;
}
// initEnvs (PPO_Discrete.cpp:365-402) from a device array: NEXT_OBS = obs, NEXT_DONE = 0, per-env episode sums = 0, in stream order
extern "C" ppo_status ppo_dev_env_reset(ppo_ctx* c, const float* obs, void* caller_stream) {
    NEED(c, c != nullptr, "null ctx");
    ppo_status s = host_state(c, "ppo_dev_env_reset");
    if (s != PPO_OK) return s;
    if (c->host_phase != 0) return fail(c, PPO_ERR_STATE, "ppo_dev_env_reset: a rollout is open (ppo_host_rollout_end first)");
    NEED(c, obs != nullptr, "ppo_dev_env_reset: null argument");
    DeviceGuard dev_guard(c);
    hipStream_t caller = static_cast<hipStream_t>(caller_stream);
    s = dev_handover_in(c, caller);
    if (s != PPO_OK) return s;
    s = reset_episode_state(c);
    if (s != PPO_OK) return s;
    if (c->on_mode != 0) {
        s = on_batch(c, obs, B_<float>(c, PPO_BUF_NEXT_OBS), c->N);
        if (s != PPO_OK) return s;
    } else {
        HIPCHK(c, hipMemcpyAsync(c->buf[PPO_BUF_NEXT_OBS], obs, (size_t)c->N * c->O * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    }
    return dev_handover_out(c, caller);
}

// how a device-fed act ends: the hand-over back to the caller's stream, and the state behind the enqueue
static ppo_status dev_acted(ppo_ctx* c, hipStream_t caller) {
    const ppo_status s = dev_handover_out(c, caller);
    if (s != PPO_OK) return s;
    if (c->host_feed == 0) {   // the first act: this rollout is device-fed, and its events go to the other list
        c->host_feed = 2;
        c->dev_list ^= 1;
        c->dev_list_used = false;
    }
    c->host_t += 1;
    c->host_phase = 2;
    return PPO_OK;
}

// Step t on the committed state (NEXT_OBS / NEXT_DONE); the i64 actions go to the caller's device array with plain stores
extern "C" ppo_status ppo_dev_act(ppo_ctx* c, const uint8_t* mask, int64_t* action, void* caller_stream) {
    NEED(c, c != nullptr, "null ctx");
    ppo_status s = dev_state(c, "ppo_dev_act");
    if (s != PPO_OK) return s;
    if (is_gauss(c)) return wrong_action_type(c, "ppo_dev_act", "ppo_dev_act_f32");
    if (c->host_phase == 0) return fail(c, PPO_ERR_STATE, "ppo_dev_act: no rollout is open (ppo_host_rollout_begin)");
    if (c->host_phase == 2) return fail(c, PPO_ERR_STATE, "ppo_dev_act: step %d was acted on and not observed (ppo_dev_observe)", c->host_t - 1);
    if (c->host_t >= c->T) return fail(c, PPO_ERR_STATE, "ppo_dev_act: all %d steps of the rollout are taken (ppo_host_rollout_end)", c->T);
    NEED(c, action != nullptr, "ppo_dev_act: null argument");
    DeviceGuard dev_guard(c);
    hipStream_t caller = static_cast<hipStream_t>(caller_stream);
    s = dev_handover_in(c, caller);
    if (s != PPO_OK) return s;
    // commit = 0: ppo_dev_observe committed step t - 1.  The caller's mask is read in place, and its action array is also what the rollout stores read.
    s = act_slice(c, StepSlice{ c->host_t, 0, c->N, false, false }, c->cfg.dist_kind == PPO_DIST_MASKED ? mask : nullptr, action);
    if (s != PPO_OK) return s;
    return dev_acted(c, caller);
}

// ppo_dev_act for a Gaussian context: the f32 actions [N,D] go straight to the caller's device array, and the rollout stores read them there
extern "C" ppo_status ppo_dev_act_f32(ppo_ctx* c, float* action, void* caller_stream) {
    NEED(c, c != nullptr, "null ctx");
    ppo_status s = dev_state(c, "ppo_dev_act_f32");
    if (s != PPO_OK) return s;
    if (!is_gauss(c)) return wrong_action_type(c, "ppo_dev_act_f32", "ppo_dev_act");
    if (c->host_phase == 0) return fail(c, PPO_ERR_STATE, "ppo_dev_act_f32: no rollout is open (ppo_host_rollout_begin)");
    if (c->host_phase == 2) return fail(c, PPO_ERR_STATE, "ppo_dev_act_f32: step %d was acted on and not observed (ppo_dev_observe)", c->host_t - 1);
    if (c->host_t >= c->T) return fail(c, PPO_ERR_STATE, "ppo_dev_act_f32: all %d steps of the rollout are taken (ppo_host_rollout_end)", c->T);
    NEED(c, action != nullptr, "ppo_dev_act_f32: null argument");
    DeviceGuard dev_guard(c);
    hipStream_t caller = static_cast<hipStream_t>(caller_stream);
    s = dev_handover_in(c, caller);
    if (s != PPO_OK) return s;
    s = act_slice_f32(c, StepSlice{ c->host_t, 0, c->N, false, false }, action);   // commit = 0, as in ppo_dev_act
    if (s != PPO_OK) return s;
    return dev_acted(c, caller);
}

// stepEnvs' outputs for step t (:413-483) from device arrays, committed at once: one launch, and the fold launch behind it when flags are passed
extern "C" ppo_status ppo_dev_observe(ppo_ctx* c, const float* next_obs, const float* reward, const int32_t* done, const int32_t* fin_len, const float* fin_rew,
                                      const int32_t* truncated, const float* final_obs, void* caller_stream) {
    NEED(c, c != nullptr, "null ctx");
    ppo_status s = dev_state(c, "ppo_dev_observe");
    if (s != PPO_OK) return s;
    if (c->host_phase != 2) return fail(c, PPO_ERR_STATE, "ppo_dev_observe: no step awaits its observation (ppo_dev_act first)");
    NEED(c, next_obs && reward && done, "ppo_dev_observe: null argument");
    NEED(c, (fin_len == nullptr) == (fin_rew == nullptr), "ppo_dev_observe: fin_len and fin_rew: both or neither");
    NEED(c, truncated == nullptr || final_obs != nullptr, "ppo_dev_observe: truncated is given and final_obs is null");
    if (truncated && c->gen && !c->gauss_fused && !c->cat_fused)   // the two fused families have ONE critic kernel, whatever the row count: they fold below
        return fail(c, PPO_ERR_UNSUPPORTED, "ppo_dev_observe: truncation flags on a generic network (its critic launch is chosen by a row count the host does not "
                                            "have here); fold with ppo_bootstrap_rewards where the count is known");
    DeviceGuard dev_guard(c);
    hipStream_t caller = static_cast<hipStream_t>(caller_stream);
    const int t = c->host_t - 1, N = c->N;
    if (truncated)   // both lists, T * N entries each, made by the first call that passes flags
        for (DevEventList& l : c->dev_events) {
            s = events_reserve(c, l, (int64_t)c->T * N);
            if (s != PPO_OK) return s;
        }
    HostStepArgs h = host_args(c, t + 1, false, 0, true, fin_len != nullptr);
    h.st_obs = next_obs; h.st_rew = reward; h.st_done = done; h.st_fin_len = fin_len; h.st_fin_rew = fin_rew;
    s = dev_handover_in(c, caller);
    if (s != PPO_OK) return s;
    if (c->on_mode != 0) {   // observation normalisation: the caller's rows into the context's scratch, and the commit reads the scratch
        s = on_batch(c, next_obs, c->on_obs, N);
        if (s != PPO_OK) return s;
        h.st_obs = c->on_obs;
        if (truncated) {     // the flagged rows of final_obs by the statistics of this step, not updating them; the fold reads the second scratch
            HIPCHK(c, launch_obsnorm_apply(final_obs, c->on_final, N, c->O, c->on_stats, c->on_eps, c->on_clip, truncated, done, c->stream));
            final_obs = c->on_final;
        }
    }
    s = rn_batch(c, h);   // reward normalisation: in front of the commit, so that the fold behind it adds gamma * V to the normalised reward
    if (s != PPO_OK) return s;
    HIPCHK(c, launch_host_commit(h, N, c->O, c->stream));
    if (truncated) {
        DevEventList& l = c->dev_events[c->dev_list];
        if (!c->dev_list_used) {   // in front of the rollout's first fold
            s = events_clear(c, l);
            if (s != PPO_OK) return s;
            c->dev_list_used = true;
        }
        DevFoldArgs f{};
        f.truncated = truncated; f.done = done; f.final_obs = final_obs;
        f.N = N; f.tN = (int64_t)t * N; f.gamma = c->cfg.gamma;
        f.rewards = B_<float>(c, PPO_BUF_REWARDS);
        events_sink(l, f);
        // the critic bootstrap_launch would pick for this context
        if (c->gen) {   // PPO_KERNEL_GAUSS_FUSED / PPO_KERNEL_CAT_FUSED: gen_values' kernel, counted like its launches
            c->gf_launches[1] += 1;
            HIPCHK(c, gauss_fused_dev_fold(c->gen->L, B_<float>(c, PPO_BUF_PARAMS), f, c->stream));
        } else if (critic_is_mfma(c)) HIPCHK(c, launch_dev_fold_mfma(B_<float>(c, PPO_BUF_PARAMS), c->L, f, c->stream));
        else HIPCHK(c, launch_dev_fold(B_<float>(c, PPO_BUF_PARAMS), c->L, f, c->stream));
    }
    s = dev_handover_out(c, caller);
    if (s != PPO_OK) return s;
    c->host_phase = 1;
    return PPO_OK;
}

// ---------------------------------------------------------------------------------------------------------
// Observation normalisation: the four ppo_obs_norm_* calls (ppo_hip.h).  The launches sit in ppo_host_env_reset / ppo_dev_env_reset, the acts (act_slice*),
// ppo_dev_observe, ppo_host_rollout_end and host_fold_truncations (on_batch / on_staged above).
// ---------------------------------------------------------------------------------------------------------
static ppo_status on_state(ppo_ctx* c, const char* what, bool outside_rollout) {
    if (!c->host_env)
        return fail(c, PPO_ERR_UNSUPPORTED, "%s: this context steps its own device environment (env_kind %d%s), whose observations are of unit scale and never leave "
                                            "the fused rollout; observation normalisation serves PPO_ENV_HOST contexts", what, c->cfg.env_kind, env_generic_note(c));
    if (outside_rollout && c->host_phase != 0) return fail(c, PPO_ERR_STATE, "%s: a rollout is open (ppo_host_rollout_end first)", what);
    return PPO_OK;
}

extern "C" ppo_status ppo_obs_norm_enable(ppo_ctx* c, int32_t mode, float clip, float eps) {
    NEED(c, c != nullptr, "null ctx");
    ppo_status s = on_state(c, "ppo_obs_norm_enable", true);
    if (s != PPO_OK) return s;
    if (mode < 0 || mode > 2) return fail(c, PPO_ERR_INVALID, "ppo_obs_norm_enable: mode %d (0 off, 1 update + apply, 2 apply only)", (int)mode);
    if (!(clip > 0.0f) || !(eps > 0.0f) || !std::isfinite(clip) || !std::isfinite(eps))
        return fail(c, PPO_ERR_INVALID, "ppo_obs_norm_enable: clip %g and eps %g must be positive and finite", (double)clip, (double)eps);
    if (mode != 0 && (c->cfg.global_num_envs > c->cfg.num_envs || c->world > 1 || c->comm || c->lgroup || c->xchg))
        return fail(c, PPO_ERR_UNSUPPORTED, "ppo_obs_norm_enable: this context is a shard of a multi-GPU job: per-rank statistics would make the replicas disagree");
    if (mode != 0) {
        s = on_reserve(c);
        if (s != PPO_OK) return s;
    }
    c->on_mode = mode; c->on_clip = clip; c->on_eps = eps;
    return PPO_OK;
}

extern "C" ppo_status ppo_obs_norm_get_h(ppo_ctx* c, double* mean_h, double* var_h, int64_t O, double* count) {
    NEED(c, c != nullptr, "null ctx");
    const ppo_status s = on_state(c, "ppo_obs_norm_get_h", true);
    if (s != PPO_OK) return s;
    NEED(c, mean_h && var_h && count, "ppo_obs_norm_get_h: null argument");
    if (O != c->O) return fail(c, PPO_ERR_INVALID, "ppo_obs_norm_get_h: O = %lld, the context's obs_size is %d", (long long)O, c->O);
    if (!c->on_stats) {   // never enabled, never set: the initial statistics
        for (int o = 0; o < c->O; o++) { mean_h[o] = 0.0; var_h[o] = 1.0; }
        *count = 0.0;
        return PPO_OK;
    }
    DeviceGuard dev_guard(c);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(mean_h, c->on_stats, (size_t)O * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(var_h, c->on_stats + O, (size_t)O * sizeof(double), hipMemcpyDeviceToHost));
    *count = c->on_count;
    return PPO_OK;
}

extern "C" ppo_status ppo_obs_norm_set_h(ppo_ctx* c, const double* mean_h, const double* var_h, int64_t O, double count) {
    NEED(c, c != nullptr, "null ctx");
    ppo_status s = on_state(c, "ppo_obs_norm_set_h", true);
    if (s != PPO_OK) return s;
    NEED(c, mean_h && var_h, "ppo_obs_norm_set_h: null argument");
    if (O != c->O) return fail(c, PPO_ERR_INVALID, "ppo_obs_norm_set_h: O = %lld, the context's obs_size is %d", (long long)O, c->O);
    if (!(count >= 0.0) || !std::isfinite(count)) return fail(c, PPO_ERR_INVALID, "ppo_obs_norm_set_h: count %g", count);
    for (int64_t o = 0; o < O; o++)
        if (!std::isfinite(mean_h[o]) || !(var_h[o] >= 0.0) || !std::isfinite(var_h[o]))
            return fail(c, PPO_ERR_INVALID, "ppo_obs_norm_set_h: column %lld: mean %g, var %g (finite, var >= 0)", (long long)o, mean_h[o], var_h[o]);
    s = on_reserve(c);
    if (s != PPO_OK) return s;
    DeviceGuard dev_guard(c);
    HIPCHK(c, hipStreamSynchronize(c->stream));   // nothing enqueued may still be reading the statistics
    HIPCHK(c, hipMemcpy(c->on_stats, mean_h, (size_t)O * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->on_stats + O, var_h, (size_t)O * sizeof(double), hipMemcpyHostToDevice));
    c->on_count = count;
    return PPO_OK;
}

extern "C" ppo_status ppo_obs_norm_apply(ppo_ctx* c, const float* obs, int64_t n, float* out, void* stream) {
    NEED(c, c != nullptr, "null ctx");
    ppo_status s = on_state(c, "ppo_obs_norm_apply", false);
    if (s != PPO_OK) return s;
    NEED(c, n >= 0, "ppo_obs_norm_apply: n < 0");
    if (n == 0) return PPO_OK;
    NEED(c, obs && out, "ppo_obs_norm_apply: null argument");
    s = on_reserve(c);
    if (s != PPO_OK) return s;
    DeviceGuard dev_guard(c);
    hipStream_t caller = static_cast<hipStream_t>(stream);
    s = dev_handover_in(c, caller);
    if (s != PPO_OK) return s;
    HIPCHK(c, launch_obsnorm_apply(obs, out, n, c->O, c->on_stats, c->on_eps, c->on_clip, nullptr, nullptr, c->stream));
    return dev_handover_out(c, caller);
}

// ---------------------------------------------------------------------------------------------------------
// Reward normalisation: the three ppo_reward_norm_* calls (ppo_hip.h).  The launches sit in the acts (act_slice*), ppo_dev_observe and ppo_host_rollout_end
// (rn_batch above), the accumulators are cleared by the two resets (reset_episode_state).
// ---------------------------------------------------------------------------------------------------------
static ppo_status rn_state(ppo_ctx* c, const char* what) {
    if (c->rn_ws) return PPO_OK;   // a fused device env with PPO_KERNEL_ENV_REWARD_NORM: the launches sit behind its rollout (env_normalise_rewards)
    if (!c->host_env)
        return fail(c, PPO_ERR_UNSUPPORTED, "%s: this context steps its own device environment (env_kind %d%s), whose rewards are of unit scale and never leave "
                                            "the fused rollout; reward normalisation serves PPO_ENV_HOST contexts", what, c->cfg.env_kind, env_generic_note(c));
    if (c->host_phase != 0) return fail(c, PPO_ERR_STATE, "%s: a rollout is open (ppo_host_rollout_end first)", what);
    return PPO_OK;
}

extern "C" ppo_status ppo_reward_norm_enable(ppo_ctx* c, int32_t mode, float clip, float eps) {
    NEED(c, c != nullptr, "null ctx");
    ppo_status s = rn_state(c, "ppo_reward_norm_enable");
    if (s != PPO_OK) return s;
    if (mode < 0 || mode > 2) return fail(c, PPO_ERR_INVALID, "ppo_reward_norm_enable: mode %d (0 off, 1 update + apply, 2 apply only)", (int)mode);
    if (!(clip > 0.0f) || !(eps > 0.0f) || !std::isfinite(clip) || !std::isfinite(eps))
        return fail(c, PPO_ERR_INVALID, "ppo_reward_norm_enable: clip %g and eps %g must be positive and finite", (double)clip, (double)eps);
    if (mode != 0 && (c->cfg.global_num_envs > c->cfg.num_envs || c->world > 1 || c->comm || c->lgroup || c->xchg))
        return fail(c, PPO_ERR_UNSUPPORTED, "ppo_reward_norm_enable: this context is a shard of a multi-GPU job: per-rank statistics would make the replicas disagree");
    if (mode != 0) {
        s = rn_reserve(c);
        if (s != PPO_OK) return s;
    }
    c->rn_mode = mode; c->rn_clip = clip; c->rn_eps = eps;
    return PPO_OK;
}

extern "C" ppo_status ppo_reward_norm_get_h(ppo_ctx* c, double* mean, double* var, double* count, double* ret_h, int64_t N) {
    NEED(c, c != nullptr, "null ctx");
    const ppo_status s = rn_state(c, "ppo_reward_norm_get_h");
    if (s != PPO_OK) return s;
    NEED(c, mean && var && count, "ppo_reward_norm_get_h: null argument");
    if (ret_h && N != c->N) return fail(c, PPO_ERR_INVALID, "ppo_reward_norm_get_h: N = %lld, the context's num_envs is %d", (long long)N, c->N);
    if (!c->rn_stats) {   // never enabled, never set: the initial state
        *mean = 0.0; *var = 1.0; *count = 0.0;
        if (ret_h) std::memset(ret_h, 0, (size_t)c->N * sizeof(double));
        return PPO_OK;
    }
    DeviceGuard dev_guard(c);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    double st[2];
    HIPCHK(c, hipMemcpy(st, c->rn_stats, sizeof(st), hipMemcpyDeviceToHost));
    if (ret_h) HIPCHK(c, hipMemcpy(ret_h, c->rn_ret, (size_t)c->N * sizeof(double), hipMemcpyDeviceToHost));
    *mean = st[0]; *var = st[1]; *count = c->rn_count;
    return PPO_OK;
}

extern "C" ppo_status ppo_reward_norm_set_h(ppo_ctx* c, double mean, double var, double count) {
    NEED(c, c != nullptr, "null ctx");
    ppo_status s = rn_state(c, "ppo_reward_norm_set_h");
    if (s != PPO_OK) return s;
    if (!std::isfinite(mean) || !(var >= 0.0) || !std::isfinite(var) || !(count >= 0.0) || !std::isfinite(count))
        return fail(c, PPO_ERR_INVALID, "ppo_reward_norm_set_h: mean %g, var %g, count %g (finite, var >= 0, count >= 0)", mean, var, count);
    s = rn_reserve(c);
    if (s != PPO_OK) return s;
    DeviceGuard dev_guard(c);
    HIPCHK(c, hipStreamSynchronize(c->stream));   // nothing enqueued may still be reading the statistics
    const double st[2] = {mean, var};
    HIPCHK(c, hipMemcpy(c->rn_stats, st, sizeof(st), hipMemcpyHostToDevice));
    c->rn_count = count;
    return PPO_OK;
}

// After T act / observe pairs: commit step T - 1, the values of every stored observation and the bootstrap value (:280) in one batched launch, the
// scan and the update -- the rest of ppo_train_iteration
extern "C" ppo_status ppo_host_rollout_end(ppo_ctx* c) {
    NEED(c, c != nullptr, "null ctx");
    ppo_status s = host_state(c, "ppo_host_rollout_end");
    if (s != PPO_OK) return s;
    if (c->host_phase == 0) return fail(c, PPO_ERR_STATE, "ppo_host_rollout_end: no rollout is open (ppo_host_rollout_begin)");
    for (int g = 0; g < c->host_n_groups; g++) {
        const ppo_ctx::HostGroup& G = c->host_grp[g];
        if (G.t != c->T || !G.staged)
            return fail(c, PPO_ERR_STATE, "ppo_host_rollout_end: group %d: %d of %d steps acted on, %d observed", g, G.t, c->T, G.staged ? G.t : (G.t > 0 ? G.t - 1 : 0));
    }
    const bool dev_fed = c->host_feed == 2;   // every step was committed by its ppo_dev_observe; the events were folded there
    const bool observed = dev_fed ? c->host_phase == 1 : c->host_staged;
    if (c->host_n_groups == 0 && (c->host_t != c->T || !observed))
        return fail(c, PPO_ERR_STATE, "ppo_host_rollout_end: %d of %d steps acted on, %d observed", c->host_t, c->T, observed ? c->host_t : (c->host_t > 0 ? c->host_t - 1 : 0));
    DeviceGuard dev_guard(c);
    const int N = c->N, T = c->T;
    if (dev_fed) {
        if (c->dev_list_used) {   // in front of the value launch: ppo_host_truncations waits for the folds only
            s = events_close(c, c->dev_events[c->dev_list]);
            if (s != PPO_OK) return s;
        }
    } else if (c->host_n_groups > 0) {   // every group's step T - 1 in one launch
        HostGroupTable tab{};
        tab.n = c->host_n_groups;
        for (int g = 0; g < tab.n; g++) { tab.row0[g] = c->host_grp[g].row0; tab.fin_given[g] = c->host_grp[g].fin_given ? 1 : 0; }
        tab.row0[tab.n] = N;
        HIPCHK(c, launch_host_commit_groups(host_args(c, T, false, 0, true, false), tab, N, c->O, c->stream));
    } else {
        HostStepArgs h = host_args(c, T, false, 0, c->host_staged, c->host_fin_given);
        s = on_staged(c, h);
        if (s != PPO_OK) return s;
        s = rn_batch(c, h);
        if (s != PPO_OK) return s;
        HIPCHK(c, launch_host_commit(h, N, c->O, c->stream));
    }
    float* next_obs = B_<float>(c, PPO_BUF_NEXT_OBS);
    if (c->gen) {
        s = gen_values(c, B_<float>(c, PPO_BUF_OBS), (int64_t)T * N, B_<float>(c, PPO_BUF_VALUES));
        if (s == PPO_OK) s = gen_values(c, next_obs, N, B_<float>(c, PPO_BUF_NEXT_VALUE));
        if (s != PPO_OK) return s;
    } else if (critic_is_mfma(c)) {   // launch_rollout's tail
        HIPCHK(c, launch_values_mfma(B_<float>(c, PPO_BUF_PARAMS), c->L, B_<float>(c, PPO_BUF_OBS), (int64_t)T * N, B_<float>(c, PPO_BUF_VALUES), next_obs, N,
                                     B_<float>(c, PPO_BUF_NEXT_VALUE), c->stream));
    } else {
        HIPCHK(c, launch_values(B_<float>(c, PPO_BUF_PARAMS), c->L, B_<float>(c, PPO_BUF_OBS), (int64_t)T * N, B_<float>(c, PPO_BUF_VALUES), next_obs, N,
                                B_<float>(c, PPO_BUF_NEXT_VALUE), c->stream));
    }
    c->host_phase = 0;
    c->host_staged = false;
    c->host_n_groups = 0;
    c->rollout_steps += T;
    c->global_step += (int64_t)T * c->cfg.global_num_envs;   // :526
    c->fin_pending = true;
    c->host_feed = 0;
    if (dev_fed) {
        c->dev_last = c->dev_list_used ? c->dev_list : -1;
        c->dev_list_used = false;
        c->trunc_last_idx.clear();   // (no host-side event can be pending: trunc_n == 0)
    } else {
        c->dev_last = -1;
        s = host_fold_truncations(c);   // (FIN_REW, EP_REW and the episode statistics were committed above: they keep the raw rewards)
        if (s != PPO_OK) return s;
    }
    s = run_scan(c);
    if (s != PPO_OK) return s;
    return ppo_update(c);
}

// Statistics are read in two steps so that reading them does not have to drain the stream:
//   ppo_stats_snapshot       enqueues, behind everything enqueued so far, asynchronous copies of every device piece the statistics are made of into
//                            ONE pinned host block, records an event, and notes the host-side training state (learning rate, step counters);
//   ppo_stats_snapshot_read  waits for THAT event (not for the stream) and decodes the block.
// A host that prints a table per update (the facade's train()) takes the snapshot right behind ppo_update, enqueues the next iteration, and only then
// reads: the GPU works through iteration k + 1 while the host formats iteration k.  ppo_read_stats = snapshot + read.
extern "C" ppo_status ppo_stats_snapshot(ppo_ctx* c) {
    NEED(c, c != nullptr, "null ctx");
    DeviceGuard dev_guard(c);
    ppo_status s = consume_finished_episodes(c);
    if (s != PPO_OK) return s;
    if (c->snap_count == 2) return fail(c, PPO_ERR_STATE, "two statistics snapshots are pending: read one (ppo_stats_snapshot_read) before taking a third");
    const int slot = (c->snap_oldest + c->snap_count) & 1;
    StatsSnap* h = c->snap + slot;
    h->have_step = c->last_stat_slot >= 0;
    h->have_ev = c->have_ev;
    h->have_gstats = c->have_gstats;
    h->world = c->world; h->B = c->B; h->global_step = c->global_step; h->opt_step = c->opt_step; h->updates = c->updates; h->lr = c->lr;
    h->xchg_flag = 0;
    h->es_applied = h->es_nominal = 0;
    if (c->es_pending) {   // an update with a target KL whose outcome the host has not seen: the applied-step count its epilogue forms rides along
        h->es_nominal = c->es_nominal;
        HIPCHK(c, hipMemcpyAsync(&h->es_applied, &c->es_dev->applied_total, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipMemcpyAsync(&h->error_flag, c->error_flag, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (c->xchg && c->xchg->timeout_flag) HIPCHK(c, hipMemcpyAsync(&h->xchg_flag, c->xchg->timeout_flag, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (h->have_step) HIPCHK(c, hipMemcpyAsync(&h->st, c->step_stats + c->last_stat_slot, sizeof h->st, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(h->cf, c->clipfrac_accum, sizeof h->cf, hipMemcpyDeviceToHost, c->stream));
    if (h->have_gstats) HIPCHK(c, hipMemcpyAsync(h->gstats, c->gstats, sizeof h->gstats, hipMemcpyDeviceToHost, c->stream));
    else {
        if (h->have_ev) HIPCHK(c, hipMemcpyAsync(h->ev, c->ev_sums, sizeof h->ev, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(&h->ring, c->ring, sizeof h->ring, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipEventRecord(c->snap_ev[slot], c->stream));
    c->snap_count += 1;
    return PPO_OK;
}

extern "C" ppo_status ppo_stats_snapshot_read(ppo_ctx* c, ppo_stats* out) {
    NEED(c, c && out, "null argument");
    DeviceGuard dev_guard(c);
    NEED(c, c->snap_count > 0, "no statistics snapshot is pending (ppo_stats_snapshot)");
    std::memset(out, 0, sizeof *out);
    const int slot = c->snap_oldest;
    HIPCHK(c, hipEventSynchronize(c->snap_ev[slot]));
    c->snap_oldest ^= 1;
    c->snap_count -= 1;
    StatsSnap& h = c->snap[slot];
    h.error_flag &= ~PPO_ERRFLAG_NOT_ERRORS;   // the KL gate's stop is not an error (and an update has cleared it by the time a snapshot behind it is taken)
    if (h.error_flag & 1) return fail(c, PPO_ERR_STATE, "CartPole reset-stream table exhausted (capacity %d resets per env)", c->reset_cap);
    if (h.error_flag & PPO_ERRFLAG_ROLLOUT_RANGE)
        return fail(c, PPO_ERR_STATE, "rollout: an output-layer weight of the actor is >= 255 in magnitude and does not fit the fp16 operand of the matrix-core rollout "
                                      "(its logits are invalid): create the context with PPO_KERNEL_ROLLOUT_VECTOR in ppo_config.kernel_flags");
    if (h.error_flag & PPO_ERRFLAG_UPDATE_PROTOCOL)
        return fail(c, PPO_ERR_STATE, "update kernel: a bounded wait between its forward and gradient waves ran out (the gradient of that step was incomplete: "
                                      "parameters are undefined from there on)");
    if (h.error_flag & PPO_ERRFLAG_GAE_PROTOCOL)
        return fail(c, PPO_ERR_STATE, "advantage scan: a bounded wait between the mover waves and the walker of the time-pipelined kernel ran out (the advantages and "
                                      "returns of that strip of envs are NaN, and so is everything trained on them)");
    if (h.error_flag & PPO_ERRFLAG_UPDATE_RANGE)
        return fail(c, PPO_ERR_STATE, "update kernel: an observation of magnitude >= 65504 does not fit the fp16 operand of the matrix-core update kernel; the optimizer "
                                      "gradient of that update is not finite and the parameters are undefined from there on: create the context with "
                                      "PPO_KERNEL_UPDATE_VECTOR in ppo_config.kernel_flags");
    if (h.xchg_flag != 0)
        return fail(c, PPO_ERR_COMM, "direct exchange: an all-reduce gave up waiting for a peer after %.1f s; its sums were incomplete, the replicas have "
                                     "diverged and the communicator is dead (every later all-reduce returns at once)", c->xchg ? c->xchg->wait_seconds : 0.0);
    if (h.have_step) {
        const StepStats& st = h.st;
        out->pg_loss = st.pg_loss; out->v_loss = st.v_loss; out->entropy_loss = st.entropy_loss; out->approx_kl = st.approx_kl;
        out->loss = st.loss; out->clipfrac_last = st.clipfrac; out->total_norm = st.total_norm;
    }
    out->clipfrac_mean = h.cf[1] > 0 ? h.cf[0] / h.cf[1] : 0.0;
    if (h.have_gstats) {
        // sharded: the all-reduced block of the last ppo_update holds every rank's explained-variance sums and ring -- the same bytes on every rank
        const double* g = h.gstats;
        const double n = (double)h.B * h.world;
        const double var_y = (g[1] - g[0] * g[0] / n) / (n - 1.0), var_d = (g[3] - g[2] * g[2] / n) / (n - 1.0);
        out->explained_variance = (double)(1.0f - (float)var_d / (float)var_y);  // :647-648 over the job's whole batch
        // the job's CircularBuffer(100): the newest 100 episodes of the union, in the reference's push order (step, then global env index)
        struct Ep { double key, len, rew; };
        std::vector<Ep> eps;
        double total = 0;
        for (int r = 0; r < h.world; r++) {
            const double* slot = g + PPO_GSTAT_HEAD + (size_t)r * PPO_GSTAT_RANK;
            total += slot[0];
            const int size = (int)slot[1];
            for (int i = 0; i < size && i < 100; i++) eps.push_back({ slot[4 + 3 * i], slot[4 + 3 * i + 1], slot[4 + 3 * i + 2] });
        }
        std::sort(eps.begin(), eps.end(), [](const Ep& a, const Ep& b) { return a.key < b.key; });
        const size_t keep = std::min<size_t>(eps.size(), 100), first = eps.size() - keep;
        if (keep > 0) {
            // the reference sums the ring from slot 0 upwards (Utils.h:72-78): lay the merged episodes out as the single ring would hold them --
            // episode number j of the job sits in slot j % 100
            std::vector<Ep> ring_order(keep);
            for (size_t i = 0; i < keep; i++) {
                const long long j = (long long)total - (long long)keep + (long long)i;   // 0-based episode number
                ring_order[keep < 100 ? i : (size_t)(j % 100)] = eps[first + i];
            }
            double sl = 0, sr = 0;
            for (size_t i = 0; i < keep; i++) { sl += ring_order[i].len; sr += ring_order[i].rew; }
            out->ep_len_mean = sl / (double)keep;
            out->ep_rew_mean = (double)(float)(sr / (double)keep);
        }
        out->ep_count = (int32_t)keep;
    } else {
        if (h.have_ev) {
            double sy = 0, sy2 = 0, sd = 0, sd2 = 0;
            for (int b = 0; b < PPO_EV_BLOCKS; b++) { sy += h.ev[b * 4]; sy2 += h.ev[b * 4 + 1]; sd += h.ev[b * 4 + 2]; sd2 += h.ev[b * 4 + 3]; }
            const double n = (double)h.B;
            const double var_y = (sy2 - sy * sy / n) / (n - 1.0), var_d = (sd2 - sd * sd / n) / (n - 1.0);
            out->explained_variance = (double)(1.0f - (float)var_d / (float)var_y);  // :647-648 (float tensors)
        }
        const EpisodeRing& ring = h.ring;
        if (ring.size > 0) {
            double sl = 0, sr = 0;
            for (int i = 0; i < ring.size; i++) { sl += ring.len[i]; sr += ring.rew[i]; }
            out->ep_len_mean = sl / ring.size;                 // CircularBuffer::avgLength (Utils.h:76-78)
            out->ep_rew_mean = (double)(float)(sr / ring.size); // avgReward returns float (Utils.h:72-74)
        }
        out->ep_count = ring.size;
    }
    out->learning_rate = h.lr;
    out->global_step = h.global_step;
    out->optimizer_steps = h.opt_step - (h.es_nominal - h.es_applied);   // applied steps
    out->updates = h.updates;
    return PPO_OK;
}

extern "C" ppo_status ppo_read_stats(ppo_ctx* c, ppo_stats* out) {
    NEED(c, c && out, "null argument");
    NEED(c, c->snap_count == 0, "a statistics snapshot is pending: read it (ppo_stats_snapshot_read) before ppo_read_stats");
    ppo_status s = ppo_stats_snapshot(c);
    if (s != PPO_OK) return s;
    s = ppo_stats_snapshot_read(c, out);
    if (s != PPO_OK) return s;
    // callers rely on ppo_read_stats leaving the stream idle (it always synchronised)
    DeviceGuard dev_guard(c);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PPO_OK;
}

// ---------------------------------------------------------------------------------------------------------
// Measurement
// ---------------------------------------------------------------------------------------------------------
extern "C" ppo_status ppo_profile_enable(ppo_ctx* c, int32_t on) {
    NEED(c, c != nullptr, "null ctx");
    DeviceGuard dev_guard(c);
    // on: 0 = off, 1 = every instrumented launch, 2 = only the dominant kernel (fwd/bwd; one launch in 8) and the GAE scan,
    //     3 = in-kernel phase stamps of the dominant kernel (diagnostic variant: read its SHARES, never its run time),
    //     4 = as 2 with one launch in 41 (about one per update, a different step of the update every time)
    const bool sampled = on == 2 || on == 4;
    c->profiling = (on == 0 || on == 3) ? 0u : (sampled ? ((1u << PROF_FWD_BWD) | (1u << PROF_GAE) | (1u << PROF_ALLREDUCE)) : 0xffffffffu);
    c->prof_every = on == 2 ? 8 : (on == 4 ? 41 : 1);   // modes 2 / 4 sample the update kernel (5 / ~1 of an update's 40 launches), every GAE launch
    c->prof_count = 0;
    c->stamping = on == 3;
    if (c->profiling) {   // events are created here, not inside the region being timed
        while (c->event_pool.size() < 256) {
            hipEvent_t e = nullptr;
            HIPCHK(c, hipEventCreate(&e));
            c->event_pool.push_back(e);
        }
    }
    if (c->stamping) HIPCHK(c, hipMemsetAsync(c->stamps, 0, 24 * sizeof(unsigned long long), c->stream));
    return PPO_OK;
}

extern "C" ppo_status ppo_profile_read(ppo_ctx* c, ppo_profile* out) {
    NEED(c, c && out, "null argument");
    DeviceGuard dev_guard(c);
    std::memset(out, 0, sizeof *out);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    {
        const ppo_status hs = comm_health(c);
        if (hs != PPO_OK) return hs;
    }
    int64_t* cnt[PROF_KINDS_] = { &out->fwd_bwd_launches, &out->gae_launches, &out->rollout_launches, &out->optimizer_launches, &out->reduce_launches, &out->allreduce_launches };
    double* ms[PROF_KINDS_] = { &out->fwd_bwd_ms, &out->gae_ms, &out->rollout_ms, &out->optimizer_ms, &out->reduce_ms, &out->allreduce_ms };
    for (auto& sp : c->spans) {
        float t = 0.0f;
        HIPCHK(c, hipEventElapsedTime(&t, sp.a, sp.b));
        *cnt[sp.kind] += 1;
        *ms[sp.kind] += (double)t;
        c->event_pool.push_back(sp.a);
        c->event_pool.push_back(sp.b);
    }
    c->spans.clear();
    unsigned long long st[24];
    HIPCHK(c, hipMemcpy(st, c->stamps, sizeof st, hipMemcpyDeviceToHost));
    for (int i = 0; i < 24; i++) out->phase_cycles[i] = (double)st[i];
    out->vector_fallback_launches = c->vector_fallback_launches;
    return PPO_OK;
}

// ---------------------------------------------------------------------------------------------------------
// Multi-GPU
// ---------------------------------------------------------------------------------------------------------
static ppo_status on_refuses_comm(ppo_ctx* c, const char* what) {
    return fail(c, PPO_ERR_UNSUPPORTED, "%s: observation normalisation is on (ppo_obs_norm_enable): per-rank statistics would make the replicas disagree", what);
}
static ppo_status rn_refuses_comm(ppo_ctx* c, const char* what) {
    return fail(c, PPO_ERR_UNSUPPORTED, "%s: reward normalisation is on (ppo_reward_norm_enable): per-rank statistics would make the replicas disagree", what);
}
extern "C" ppo_status ppo_comm_unique_id(void* id_out_h) {
    if (!id_out_h) return PPO_ERR_INVALID;
    std::string err;
    if (!rccl::load(err)) { g_create_error = err; return PPO_ERR_COMM; }
    rccl::UniqueId id;
    std::memset(&id, 0, sizeof id);
    const int rc = rccl::GetUniqueId(&id);
    if (rc != 0) { g_create_error = "ncclGetUniqueId failed"; return PPO_ERR_COMM; }
    static_assert(sizeof(rccl::UniqueId) == PPO_COMM_ID_BYTES, "unique id size");
    std::memcpy(id_out_h, &id, sizeof id);
    return PPO_OK;
}

extern "C" ppo_status ppo_comm_init(ppo_ctx* c, const void* id_h, int32_t rank, int32_t nranks) {
    if (c && c->on_mode != 0) return on_refuses_comm(c, "ppo_comm_init");
    if (c && c->rn_mode != 0) return rn_refuses_comm(c, "ppo_comm_init");
    NEED(c, c && id_h, "null argument");
    DeviceGuard dev_guard(c);
    NEED(c, nranks >= 1 && rank >= 0 && rank < nranks, "bad rank / nranks");
    NEED(c, nranks <= 8, "more than 8 ranks: the job-global statistics block (ppo_read_stats) and the transports serve the 8 GPUs of one node");
    NEED(c, c->cfg.global_num_envs == (int64_t)c->cfg.num_envs * nranks, "global_num_envs must equal num_envs * nranks (equal shards)");
    // ppo_config.kernel_flags & PPO_KERNEL_COMM_SELFTEST: a ONE-rank communicator is really created and every collective of the multi-rank path is
    // really issued (sums over one rank = identity): the RCCL calls on a box with a single GPU
    const bool selftest = nranks == 1 && (c->cfg.kernel_flags & PPO_KERNEL_COMM_SELFTEST) != 0;
    if (nranks == 1 && !selftest) { c->world = 1; c->rank = 0; return PPO_OK; }
    std::string err;
    if (!rccl::load(err)) return fail(c, PPO_ERR_COMM, "%s", err.c_str());
    rccl::UniqueId id;
    std::memcpy(&id, id_h, sizeof id);
    HIPCHK(c, hipSetDevice(c->cfg.device));
    const int rc = rccl::CommInitRank(&c->comm, nranks, id, rank);
    if (rc != 0) return fail(c, PPO_ERR_COMM, "ncclCommInitRank failed: %s", rccl::GetErrorString ? rccl::GetErrorString(rc) : "?");
    c->world = nranks;
    c->rank = rank;
    c->force_collectives = selftest;
    return PPO_OK;
}

// Joins the in-process group `group_id` as rank `rank` of `nranks` (all members live in this process, one host thread each).
extern "C" ppo_status ppo_comm_init_local(ppo_ctx* c, int64_t group_id, int32_t rank, int32_t nranks) {
    if (c && c->on_mode != 0) return on_refuses_comm(c, "ppo_comm_init_local");
    if (c && c->rn_mode != 0) return rn_refuses_comm(c, "ppo_comm_init_local");
    NEED(c, c != nullptr, "null ctx");
    DeviceGuard dev_guard(c);
    NEED(c, nranks >= 1 && nranks <= 8 && rank >= 0 && rank < nranks, "bad rank / nranks (in-process groups hold at most 8 contexts)");
    NEED(c, c->cfg.global_num_envs == (int64_t)c->cfg.num_envs * nranks, "global_num_envs must equal num_envs * nranks (equal shards)");
    NEED(c, c->comm == nullptr && !c->lgroup, "context already has a communicator");
    if (nranks == 1) { c->world = 1; c->rank = 0; return PPO_OK; }
    std::shared_ptr<LocalGroup> g;
    {
        std::lock_guard<std::mutex> lk(g_local_groups_mu);
        auto it = g_local_groups.find(group_id);
        if (it == g_local_groups.end()) {
            g = std::make_shared<LocalGroup>();
            g->n = nranks;
            g->device = c->cfg.device;
            HIPCHK(c, hipSetDevice(c->cfg.device));   // the group's events belong to its device
            HIPCHK(c, hipEventCreateWithFlags(&g->done[0], hipEventDisableTiming));
            HIPCHK(c, hipEventCreateWithFlags(&g->done[1], hipEventDisableTiming));
            g_local_groups[group_id] = g;
        } else {
            g = it->second;
        }
        NEED(c, g->n == nranks, "group was created with a different size");
        // one kernel on one device reads every member's buffer and the members wait on shared events: all of that is per device.  Several GPUs
        // are driven by one process per GPU (ppo_comm_init / ppo_comm_init_exchange)
        NEED(c, g->device == c->cfg.device, "in-process groups hold contexts of ONE device; use one process per GPU for several");
        if (++g->joined == g->n) g_local_groups.erase(group_id);  // complete: the id may be reused by a later group
    }
    HIPCHK(c, hipEventCreateWithFlags(&c->lg_ready, hipEventDisableTiming));
    c->lgroup = g;
    c->world = nranks;
    c->rank = rank;
    return PPO_OK;
}

// ---- one-shot direct exchange (see ExchangeComm) ----
// Step 1 (every rank): allocate the exchange buffer and export its IPC handle.  payload capacity: the larger of the gradient (+ 8 loss sums) and the
// advantage sums of one update.
extern "C" ppo_status ppo_comm_exchange_handle(ppo_ctx* c, void* handle_out_h) {
    NEED(c, c && handle_out_h, "null argument");
    DeviceGuard dev_guard(c);
    NEED(c, c->comm == nullptr && !c->lgroup, "context already has a communicator");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    if (!c->xchg) {
        std::unique_ptr<ExchangeComm> x(new ExchangeComm());
        const size_t grad = ((size_t)c->L.P + 8) * sizeof(float), adv = ((size_t)PPO_GSTAT_DOUBLES + (size_t)2 * c->steps_per_update * PPO_ADV_PARTS) * sizeof(double);   // [statistics block | advantage sums]
        x->slot_bytes = (std::max(grad, adv) + 255) / 256 * 256;
        const size_t total = 16 * x->slot_bytes + 256;   // [2 parities][8 source ranks] payload slots, 16 flags, 2 counters (kernels_update.hip: xchg_slot)
        // fine-grained device memory: stores of a running kernel become visible to peers' running kernels (coarse-grained memory is only
        // coherent at kernel boundaries); plain hipMalloc as a fallback on a single device
        hipError_t e = hipExtMallocWithFlags(&x->own, total, hipDeviceMallocFinegrained);
        if (e != hipSuccess) { (void)hipGetLastError(); HIPCHK(c, hipMalloc(&x->own, total)); }
        HIPCHK(c, hipMemset(x->own, 0, total));
        HIPCHK(c, dalloc(c, &x->timeout_flag, 4));
        const unsigned long long ticks = (unsigned long long)(x->wait_seconds * 1e8);   // s_memrealtime: 100 MHz
        HIPCHK(c, hipMemcpy(x->timeout_flag + 2, &ticks, sizeof ticks, hipMemcpyHostToDevice));
        HIPCHK(c, hipDeviceSynchronize());
        c->xchg = std::move(x);
    }
    static_assert(sizeof(hipIpcMemHandle_t) <= PPO_COMM_HANDLE_BYTES, "IPC handle size");
    hipIpcMemHandle_t h;
    HIPCHK(c, hipIpcGetMemHandle(&h, c->xchg->own));
    std::memset(handle_out_h, 0, PPO_COMM_HANDLE_BYTES);
    std::memcpy(handle_out_h, &h, sizeof h);
    return PPO_OK;
}

// Step 2 (every rank, after all handles have been gathered, e.g. over torch.distributed): map the peers' buffers and switch the context's
// all-reduces to the exchange.  handles_h: nranks x PPO_COMM_HANDLE_BYTES in rank order.
extern "C" ppo_status ppo_comm_init_exchange(ppo_ctx* c, const void* handles_h, int32_t rank, int32_t nranks) {
    if (c && c->on_mode != 0) return on_refuses_comm(c, "ppo_comm_init_exchange");
    if (c && c->rn_mode != 0) return rn_refuses_comm(c, "ppo_comm_init_exchange");
    NEED(c, c && handles_h, "null argument");
    DeviceGuard dev_guard(c);
    NEED(c, nranks >= 1 && nranks <= 8 && rank >= 0 && rank < nranks, "bad rank / nranks (the direct exchange serves the 8 GPUs of one node)");
    NEED(c, c->cfg.global_num_envs == (int64_t)c->cfg.num_envs * nranks, "global_num_envs must equal num_envs * nranks (equal shards)");
    NEED(c, c->xchg && c->xchg->own, "call ppo_comm_exchange_handle first");
    HIPCHK(c, hipSetDevice(c->cfg.device));
    ExchangeComm& x = *c->xchg;
    for (int r = 0; r < nranks; r++) {
        if (r == rank) { x.peer[r] = x.own; continue; }
        hipIpcMemHandle_t h;
        std::memcpy(&h, static_cast<const char*>(handles_h) + (size_t)r * PPO_COMM_HANDLE_BYTES, sizeof h);
        HIPCHK(c, hipIpcOpenMemHandle(&x.peer[r], h, hipIpcMemLazyEnablePeerAccess));
        x.opened[r] = true;
    }
    c->world = nranks;
    c->rank = rank;
    c->force_collectives = nranks == 1;   // a one-rank exchange still runs the multi-rank code path (self-test)
    return PPO_OK;
}

// How long a kernel of the direct exchange waits for a peer's share before it gives up (default 30 s).  Call after ppo_comm_exchange_handle.
extern "C" ppo_status ppo_comm_set_wait_limit(ppo_ctx* c, double seconds) {
    NEED(c, c != nullptr, "null ctx");
    DeviceGuard dev_guard(c);
    NEED(c, c->xchg && c->xchg->timeout_flag, "call ppo_comm_exchange_handle first");
    NEED(c, seconds >= 1e-3 && seconds <= 3600.0, "wait limit must lie in [1 ms, 1 h]");
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->xchg->wait_seconds = seconds;
    const unsigned long long ticks = (unsigned long long)(seconds * 1e8);
    HIPCHK(c, hipMemcpy(c->xchg->timeout_flag + 2, &ticks, sizeof ticks, hipMemcpyHostToDevice));
    return PPO_OK;
}

// 0: no all-reduce kernel of this context has given up waiting for a peer; non-zero: at least one has (a peer died or never joined) -- read it as
// a boolean: every polling lane that gives up adds to it, and so does every later call on the dead communicator.  Never fails because of the
// flag itself (ppo_sync / ppo_read_stats / ppo_profile_read do: PPO_ERR_COMM).
extern "C" ppo_status ppo_comm_exchange_timeouts(ppo_ctx* c, int32_t* count_out) {
    NEED(c, c && count_out, "null argument");
    DeviceGuard dev_guard(c);
    *count_out = 0;
    if (!c->xchg) return PPO_OK;
    HIPCHK(c, hipMemcpyAsync(count_out, c->xchg->timeout_flag, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PPO_OK;
}
