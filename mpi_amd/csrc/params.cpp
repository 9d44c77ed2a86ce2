// params.cpp -- every knob and every diagnostic the library has, one row each: what xmpi_set_param accepts, what xmpi_get_param
// answers and what xmpi_init takes from the environment all walk this table (INTEGRATION.md section 5 is the same table in words,
// held to it by tests/test_abi.py through xmpi_param_info).
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "comm.h"

namespace xmpi {
namespace {

enum : int { W = XMPI_PARAM_WRITABLE, B = XMPI_PARAM_BOOLEAN, LAYOUT = XMPI_PARAM_LAYOUT_DEFAULT, PATTERN = XMPI_PARAM_PATTERN, AUTO = XMPI_PARAM_ENV_AUTO };
constexpr long kAny = LONG_MAX;

struct Param {
  const char* name;  // of xmpi_set_param / xmpi_get_param (null: a variable of the window layout that nothing reads back)
  const char* env;   // the variable xmpi_init reads it from, or null
  long xmpi_comm::*field;          // how the value is reached: a member of the communicator;
  long (*read)(const xmpi_comm*);  // a function (a diagnostic; a member that is not what the caller should see);
  // the fixed default, or LAYOUT: decided where the job's layout is known, and handed to param_env there.  One range [lo, hi], or B:
  // 0 / 1.  AUTO: the environment (only) may say -1 = decide later, and anything below lo says the same.  W: xmpi_set_param takes it.
  long dflt, lo, hi;
  int flags;
  void (*set_process)(int) = nullptr;  // the process-wide setter of kernel_mode / grid_cap;
  // PATTERN (`name` is a prefix): one handler for both directions (set null: the value, or -1; otherwise 0 = stored, -1 = refused)
  long (*named)(xmpi_comm*, const char*, const long*) = nullptr;
};

#define READ(expr) [](const xmpi_comm* c) -> long { return (void)c, (long)(expr); }
#define DIAG(name, expr) {name, nullptr, nullptr, READ(expr), 0, 0, 0, 0}

long heap_stat(const xmpi_comm* c, int which) {
  size_t s[3] = {0, 0, 0};
  heap_stats(c->device, &s[0], &s[1], &s[2]);
  return (long)s[which];
}

long hbm_mib(const xmpi_comm* c, bool free_mib) {  // of this rank's GPU, as the runtime reports it
  size_t fr = 0, tot = 0;
  if (hipSetDevice(c->device) != hipSuccess || hipMemGetInfo(&fr, &tot) != hipSuccess) return -1;
  return (long)((free_mib ? fr : tot) >> 20);
}

// what xmpi_init's vote left the job with: 0 = everything; bit 0 (1): the split form's data kernel runs at system scope (the XCD
// probe of THIS rank's GPU); bit 1 (2): the ranks meet on the host (some flag page could not be allocated, exported or mapped);
// bit 2 (4): no windows (some window could not be mapped: no staged step tables, no mail slots); bit 3 (8): a schedule gave wrong
// answers when the library checked it here and was taken out (tune_rejected).  xmpi_degraded() says why.
long degraded(const xmpi_comm* c) {
  // (ranks hosted by threads of one process on one GPU meet on the host by design, not by degradation; so do more than the device side is sized for)
  bool shared_gpu = false;
  for (int p = 0; p < c->size; p++) shared_gpu = shared_gpu || c->peer_coloc[p];
  return (c->body_sys == 1 && c->dsync_ok ? 1 : 0) | ((c->size > 1 && c->size <= kDsyncRanks && c->dsync && !c->dsync_ok && !shared_gpu) ? 2 : 0) |
         (c->windows_ok ? 0 : 4) | (c->rejected_why.empty() ? 0 : 8);
}

// tune_<algo|split|unroll>_<collective 0..3>_<size class>: a row of the table AUTO follows once "tuned" is 1 -- xmpi_tune's to write;
// a benchmark or a test standing in for it may
long tune_cell(xmpi_comm* c, const char* name, const long* set) {
  int coll = -1, cls = -1;
  char what[16] = {0};
  if (sscanf(name, "tune_%15[a-z]_%d_%d", what, &coll, &cls) != 3 || coll < 0 || coll >= 4 || cls < 0 || cls >= xmpi_comm::kTuneClasses) return -1;
  const std::string w = what;
  int8_t(*t)[xmpi_comm::kTuneClasses] = w == "algo" ? c->tune_algo : w == "split" ? c->tune_split : w == "unroll" ? c->tune_unroll : nullptr;
  if (!t || (set && (*set < -1 || *set >= XMPI_ALGO_COUNT))) return -1;
  if (set) t[coll][cls] = (int8_t)*set;
  return set ? 0 : t[coll][cls];
}

// schedules whose answers the library found wrong on this machine, per collective (0 allreduce, 1 allgather, 2 bcast, 3 reduce) a
// bit per candidate -- the numbering of tune_mask
long tune_rejected_of(xmpi_comm* c, const char* name, const long* set) {
  return (!set && name[14] >= '0' && name[14] <= '3' && !name[15]) ? (long)c->tune_rejected[name[14] - '0'] : -1;
}

// prof_min_ns_<kind> / prof_max_ns_<kind>: the shortest / longest sampled launch of kind 0..4 since xmpi_prof_reset
long prof_extreme(xmpi_comm* c, const char* name, const long* set) {
  const int kind = name[12] - '0';
  if (set || kind < 0 || kind >= PROF_KINDS || name[13]) return -1;
  return (long)((name[6] == 'i' ? c->prof[kind].min_ms : c->prof[kind].max_ms) * 1e6);
}

const Param kParams[] = {
    // ---- knobs: name, variable, member, reader, default, lo, hi, flags -------------------------------------------------------------
    {"timeout_s", "XMPI_TIMEOUT_S", &xmpi_comm::timeout_s, nullptr, 0, 0, kAny, W},
    {"watchdog_ms", "XMPI_WATCHDOG_MS", &xmpi_comm::watchdog_ms, nullptr, 50, 0, kAny, 0},
    {"selfcheck", "XMPI_SELFCHECK", &xmpi_comm::selfcheck, nullptr, -1, 0, 1, B | AUTO},
    {"zero_copy", "XMPI_ZERO_COPY", &xmpi_comm::zero_copy, nullptr, 1, 0, 1, W | B},
    {"dsync", "XMPI_DSYNC", &xmpi_comm::dsync, READ(dsync_usable(c) ? 1 : 0), 1, 0, 1, W | B},
    {"ll_bytes", "XMPI_LL_BYTES", &xmpi_comm::ll_bytes, nullptr, -1, 0, (long)kLLMaxPayload, W | AUTO},  // untuned AUTO: LL lines up to here
    {"agent_ll", "XMPI_AGENT_LL", &xmpi_comm::agent_ll, nullptr, 1, 0, 2, W},  // blocking LL collectives by the lingering agent (2 = 1)
    {"agent_ll_bytes", "XMPI_AGENT_LL_BYTES", &xmpi_comm::agent_ll_bytes, nullptr, 8192, 0, (long)kLLMaxPayload, W},
    {"p2p_agent_us", "XMPI_P2P_AGENT_US", &xmpi_comm::p2p_agent_us, nullptr, 40, 0, kAny, W},
    {"ll_agent_us", "XMPI_LL_AGENT_US", &xmpi_comm::ll_agent_us, nullptr, 0, 0, kAny, W | LAYOUT},  // default: p2p_agent_us as read
    {"p2p_kernel_ack", "XMPI_P2P_KERNEL_ACK", &xmpi_comm::p2p_kernel_ack, nullptr, 1, 0, 1, W | B},
    {"p2p_direct_bytes", "XMPI_P2P_DIRECT_BYTES", &xmpi_comm::p2p_direct_bytes, nullptr, 1, LONG_MIN, kAny, W},  // < 0: always the mail slots
    {"p2p_grid_cap", "XMPI_P2P_GRID_CAP", &xmpi_comm::p2p_grid_cap, nullptr, 0, 0, 4096, W},
    {"dsync_split_bytes", "XMPI_DSYNC_SPLIT_BYTES", &xmpi_comm::dsync_split_bytes, nullptr, 4 << 20, 0, kAny, W},  // 0: always one kernel
    {"dsync_unroll", "XMPI_DSYNC_UNROLL", &xmpi_comm::dsync_unroll, nullptr, 0, 1, 2, W | LAYOUT},
    {"dsync_tiles", "XMPI_DSYNC_TILES", &xmpi_comm::dsync_tiles, nullptr, 0, 1, kAny, W | LAYOUT},
    {"dsync_grid", "XMPI_DSYNC_GRID", &xmpi_comm::dsync_grid_cap, nullptr, 0, 0, kAny, W},
    {"sched_channels", "XMPI_SCHED_CHANNELS", &xmpi_comm::sched_channels, nullptr, 0, 0, kAny, W},
    {"sched_grid", "XMPI_SCHED_GRID", &xmpi_comm::sched_grid, nullptr, 0, 0, kAny, W},
    {"tree_piece_bytes", "XMPI_TREE_PIECE_BYTES", &xmpi_comm::tree_piece_bytes, nullptr, 256 << 10, 4096, kAny, W},
    {"zc_bcast_push_bytes", "XMPI_ZC_BCAST_PUSH_BYTES", &xmpi_comm::zc_bcast_push_bytes, nullptr, 256 << 10, 0, kAny, W},
    {"body_sys", "XMPI_BODY_SYS", &xmpi_comm::body_sys, nullptr, -1, 0, 1, W | B | AUTO},  // -1: decided by the XCD probe (dsync_prepare)
    {"xcd_check", "XMPI_XCD_CHECK", &xmpi_comm::xcd_check, nullptr, 1, 0, 1, W | B},
    {"tuned", nullptr, &xmpi_comm::tuned, nullptr, 0, 0, 1, W | B},  // 0: AUTO forgets the table of xmpi_tune
    // bit k = 0: xmpi_tune leaves candidate k out (xmpi_comm::CAND_*); the default form always runs
    {"tune_mask", nullptr, &xmpi_comm::tune_mask, nullptr, -1, LONG_MIN, kAny, W},
    {"prof_every", nullptr, &xmpi_comm::prof_every, nullptr, 1, 1, kAny, W},
    {"xcds", nullptr, &xmpi_comm::xcds, nullptr, 0, 0, 32, W | LAYOUT},  // probed (tests: a GPU with more XCDs than it has)
    {"channels", "XMPI_CHANNELS", &xmpi_comm::channels, nullptr, 0, 0, kAny, W},  // 0 = one ring channel per available link direction
    {"piece_bytes", "XMPI_PIECE_BYTES", &xmpi_comm::piece_bytes, nullptr, 0, 0, kAny, W},
    {"copy_engine", "XMPI_COPY_ENGINE", &xmpi_comm::copy_engine, nullptr, 0, 0, 1, W | B},
    {"batch_copies", "XMPI_BATCH_COPIES", &xmpi_comm::batch_copies, nullptr, 1, 0, 1, W | B},
    {"oneshot_bytes", "XMPI_ONESHOT_BYTES", &xmpi_comm::oneshot_bytes, nullptr, 1 << 20, 0, kAny, W},
    {"zc_group_launch", "XMPI_ZC_GROUP_LAUNCH", &xmpi_comm::zc_group_launch, nullptr, 1, 0, 1, W | B},
    {"shared_stream", "XMPI_SHARED_STREAM", nullptr, READ(c->shared_stream ? 1 : 0), -1, 0, 1, B | AUTO},  // -1: when ranks are co-located
    // the window layout (join_job: rank 0's values are the job's)
    {"lanes", "XMPI_LANES", nullptr, READ(c->lanes), 2, 1, kMaxLanes, 0},
    {"fifo_depth", "XMPI_FIFO_DEPTH", nullptr, READ(c->fifo_depth), 8, 2, 64, 0},
    {"slot_bytes", "XMPI_SLOT_BYTES", nullptr, READ(c->slot_bytes), 8l << 20, 4096, kAny, 0},
    {nullptr, "XMPI_P2P_DEPTH", nullptr, nullptr, 2, 2, 16, 0},
    {"p2p_slot_bytes", "XMPI_P2P_SLOT_BYTES", nullptr, READ(c->p2p_slot_bytes), 4l << 20, 4096, kAny, 0},
    {nullptr, "XMPI_HOST_LANES", nullptr, nullptr, 1, 0, 1, B},  // a request: the creator of the block sizes and reserves them
    // tests only (read by dsync_connect, the same on every rank; no name: nothing sets or reads them back): where the communicator's
    // epochs start at least, and how many Send / Receive messages every ordered pair counts as having exchanged already
    {nullptr, "XMPI_TEST_EPOCH_BASE", nullptr, nullptr, 0, 0, kAny, 0},
    {nullptr, "XMPI_TEST_P2P_SEQ0", nullptr, nullptr, 0, 0, kAny, 0},
    // process-wide: their own pair normalises what it is given (a mode outside 0 .. 2 is -1, a negative cap 0)
    {"kernel_mode", "XMPI_KERNEL_MODE", nullptr, READ(get_kernel_mode()), -1, -1, 2, W, set_kernel_mode},
    {"grid_cap", "XMPI_GRID_CAP", nullptr, READ(get_grid_cap()), 0, 0, INT_MAX, W, set_grid_cap},
    // ---- diagnostics -----------------------------------------------------------------------------------------------------------------
    DIAG("degraded", degraded(c)), DIAG("windows_ok", c->windows_ok ? 1 : 0),
    DIAG("dead_rank", c->ctl->dead_rank()),  // the first rank whose process the watchdog found gone; -1 = none
    // schedules whose answers the library found wrong on this machine (xmpi_tune, xmpi_init's self-check), in all
    DIAG("tune_rejected", __builtin_popcount(c->tune_rejected[0]) + __builtin_popcount(c->tune_rejected[1]) + __builtin_popcount(c->tune_rejected[2]) + __builtin_popcount(c->tune_rejected[3])),
    DIAG("p2p_rejected", c->p2p_rejected),  // the self-check's verdict on Send / Receive: bit 0 the direct pull (-> mail slots), bit 1 everything
    // xmpi_init's self-check (-1 = did not run), and of that its buffers (the job's first arena, the first kernel's code object)
    DIAG("init_selfcheck_ms", c->selfcheck_ms < 0 ? -1 : (long)(c->selfcheck_ms + 0.999)),
    DIAG("init_selfcheck_us", c->selfcheck_ms < 0 ? -1 : (long)(c->selfcheck_ms * 1e3)),
    DIAG("init_selfcheck_setup_us", c->selfcheck_ms < 0 ? -1 : (long)(c->selfcheck_setup_ms * 1e3)),
    DIAG("tune_us", c->tune_ms * 1e3), DIAG("tune_check_us", c->tune_check_ms * 1e3),  // the last xmpi_tune: all of it / the part spent checking answers
    DIAG("heap_arenas", heap_stat(c, 0)), DIAG("heap_reserved", heap_stat(c, 1)), DIAG("heap_in_use", heap_stat(c, 2)),
    DIAG("hbm_free_mib", hbm_mib(c, true)), DIAG("hbm_total_mib", hbm_mib(c, false)),
    DIAG("p2p_agent_served", c->p2p_agent_served), DIAG("p2p_agent_launches", c->p2p_agent_launches),
    DIAG("p2p_direct_count", c->p2p_direct_count), DIAG("p2p_staged_count", c->p2p_staged_count), DIAG("p2p_lane_count", c->p2p_lane_count),
    DIAG("host_bounce_calls", c->host_bounce_calls), DIAG("host_lane_bytes", c->ctl->host_lane_bytes()), DIAG("window_bytes", c->window_bytes),
    DIAG("dsync_epoch", c->dsync_epoch), DIAG("dsync_launches", c->dsync_launches), DIAG("dsync_bounced", c->dsync_bounced),
    DIAG("dsync_sharers", c->dsync_sharers), DIAG("dsync_sharers_job", c->dsync_sharers_job), DIAG("dsync_land_bytes", c->dsync_land_bytes),
    DIAG("dsync_ll_launches", c->dsync_ll_launches), DIAG("dsync_v_launches", c->dsync_v_launches), DIAG("dsync_ll_agent", c->dsync_ll_agent),
    DIAG("dsync_split_launches", c->dsync_split_launches), DIAG("dsync_sched_launches", c->dsync_sched_launches),
    DIAG("ll_max_bytes", kLLMaxPayload), DIAG("ll_agent_launches", c->ll_agent_launches), DIAG("agent_ll_wait_ns", c->agent_ll_wait_ns),  // command written -> answer seen, summed over dsync_ll_agent calls
    DIAG("roctx", roctx_enabled() ? 1 : 0),  // named ranges for the profilers are on (trace.h)
    DIAG("xcd_probe_mask", c->xcd_probe_mask), DIAG("xcd_short", c->xcd_short), DIAG("last_run_us", c->last_run_us), DIAG("last_sync_us", c->last_sync_us),
    DIAG("xcd_meet_mask", c->dsync_status ? (long)__atomic_load_n(c->dsync_status + 6, __ATOMIC_RELAXED) : -1),
    DIAG("xcd_done_mask", c->dsync_status ? (long)__atomic_load_n(c->dsync_status + 7, __ATOMIC_RELAXED) : -1),
    DIAG("zc_seq", c->zc_seq), DIAG("zc_fallbacks_unregistered", c->zc_fallbacks_unregistered), DIAG("zc_fallbacks_unmappable", c->zc_fallbacks_unmappable),
    DIAG("ring_channels_max", ring_channel_count(c->size) * c->lanes), DIAG("ring_channels", ring_channel_count(c->size)),
    // ---- patterned names: the prefix, one handler (last: an exact name wins over a prefix; the longer prefix first)
    {"tune_rejected_", nullptr, nullptr, nullptr, 0, 0, 0, PATTERN, nullptr, tune_rejected_of},
    {"tune_", nullptr, nullptr, nullptr, -1, -1, XMPI_ALGO_COUNT - 1, W | PATTERN, nullptr, tune_cell},
    {"prof_min_ns_", nullptr, nullptr, nullptr, 0, 0, 0, PATTERN, nullptr, prof_extreme},
    {"prof_max_ns_", nullptr, nullptr, nullptr, 0, 0, 0, PATTERN, nullptr, prof_extreme},
};

// the row of an exact name, else (they come last) the first PATTERN row whose prefix the name begins with
const Param* find(const char* name) {
  for (const Param& p : kParams)
    if (p.name && ((p.flags & PATTERN) ? !strncmp(p.name, name, strlen(p.name)) : !strcmp(p.name, name))) return &p;
  return nullptr;
}

// what a row makes of a value, wherever it comes from
long in_range(const Param& p, long v) {
  if (p.flags & B) return v ? 1 : 0;
  return v < p.lo ? p.lo : v > p.hi ? p.hi : v;
}

}  // namespace

// what the environment says about the row of variable `env`, in the row's range (dflt: the row's own, or what a late site computed)
long param_env(const char* env, long dflt) {
  for (const Param& p : kParams)
    if (p.env && !strcmp(p.env, env)) {
      const long v = env_long(env, dflt == kRowDefault ? p.dflt : dflt);
      return ((p.flags & AUTO) && v < p.lo) ? -1 : in_range(p, v);
    }
  return dflt;
}

void params_from_env(xmpi_comm* c) {
  for (const Param& p : kParams) {
    if (!p.env || (p.flags & LAYOUT)) continue;
    if (p.field) c->*p.field = param_env(p.env);
    else if (p.set_process && getenv(p.env)) p.set_process((int)env_long(p.env, p.dflt));
  }
}

}  // namespace xmpi

using namespace xmpi;

extern "C" {

int xmpi_set_param(xmpi_comm* c, const char* name, long value) {
  if (!c || c->finalized || !name) return XMPI_ERR_STATE;
  std::lock_guard<std::mutex> g(c->coll_mu);
  const Param* p = find(name);
  if (!p || !(p->flags & W)) return XMPI_ERR_ARG;
  if (p->named) return p->named(c, name, &value) == 0 ? XMPI_OK : XMPI_ERR_ARG;
  if (p->set_process) p->set_process((int)value);
  else c->*p->field = in_range(*p, value);
  return XMPI_OK;
}

long xmpi_get_param(const xmpi_comm* c, const char* name) {
  if (!c || c->finalized || !name) return -1;
  const Param* p = find(name);
  if (!p) return -1;
  if (p->named) return p->named(const_cast<xmpi_comm*>(c), name, nullptr);
  return p->read ? p->read(c) : c->*p->field;
}

int xmpi_param_info(int index, const char** name, const char** env, long* dflt, long* lo, long* hi, int* flags) {
  if (index < 0 || index >= (int)(sizeof kParams / sizeof kParams[0])) return XMPI_ERR_ARG;
  const Param& p = kParams[index];
  *name = p.name, *env = p.env, *dflt = p.dflt, *lo = p.lo, *hi = p.hi;
  *flags = p.flags | ((p.flags & W) ? 0 : XMPI_PARAM_READ_ONLY);
  return XMPI_OK;
}

}  // extern "C"
