// C ABI of libzkhip.so (include/zkhip.h): contexts, device buffers, registered-base residency, and the host-buffer
// wrappers around the device paths in msm.hip / ntt.hip.  No CPU arithmetic lives here.
//
// Concurrency model (callers are the thread running create_proof and possibly rayon workers):
//   * one context per HIP device named in zkhip_init; devs[0] is the PRIMARY device: every `_device` entry point, every NTT and every
//     single-shard MSM runs there.  The other devices only ever run MSM shards.
//   * scratch memory is keyed by stream.  A `_device` call uses the scratch set of the caller's stream (work on one stream is ordered,
//     so its calls may share scratch; two streams never do).  Host-buffer calls borrow a LANE -- a library-owned stream with its own
//     scratch set and pinned result buffer -- for the duration of the call and do NOT hold the library lock while they wait for the
//     device: two host threads overlap one call's PCIe transfer with the other's kernels.
//   * g_mu guards the context tables (registered bases, handles, scratch map, lanes) and the enqueue of `_device` calls.
//   * an MSM over registered bases that span several shards (zkhip_init with ndev > 1, or ZKHIP_SHARDS / zkhip_set_msm_shards virtual
//     shards on one device) fans the scalar slices out to the shards' devices, gathers the 96-byte Jacobian partials on the primary
//     device (peer copies over xGMI) and folds them there (k_sum_jacobian) -- SURVEY.md section 8(e).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <dlfcn.h>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>
#include "zkhip_internal.hpp"
#include "blake2b.hpp"
#include "poseidon.hpp"
#include "imt.hpp"
#include "modn.hpp"
#include "secp256k1_h2c.hpp"
#include "row_msm.hpp"
#include "kzg_limbs.hpp"
#include "../../include/zkhip.hpp"   // host-side 4 x 64 Montgomery arithmetic for domain constants (zkhip::halo2::detail)

namespace zkhip {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

// ---- profiler (one profiling caller at a time: a debugging aid, not part of the concurrent surface) --------------------
// mode 1: the events of the LAST call are kept (read after every call: a host read-back between calls).
// mode 2: every call appends its events to a pool and zkhip_profile_read_calls reads them all at the end, so a loop of calls runs
//         back to back as it does unprofiled (bench.py's roofline figure; round 4 read back after every call and interleaved other work,
//         which put the phase sum above the step time).
static int g_prof_mode = 0;
static const int PROF_MAX = 32;
static const int PROF_POOL = 2048;           // mode 2: events of up to PROF_POOL / 16 typical calls
static hipEvent_t g_prof_ev[PROF_POOL];
static bool g_prof_ev_ready = false;
static int g_prof_base = 0;                  // first event of the current call
static int g_prof_n = 0;                     // number of marks recorded after the current call's begin event
static char g_prof_names[PROF_POOL][24];
static int g_prof_calls[PROF_POOL / 2][2];   // mode 2: (base, marks) per recorded call
static int g_prof_ncalls = 0;
static bool g_prof_full = false;             // mode 2: the pool ran out, the current call records nothing
static bool g_prof_hold = false;             // the inner marks of a call's phase are not recorded (prof_hold)

void prof_begin(hipStream_t stream) {
  if (!g_prof_mode) return;
  if (!g_prof_ev_ready) {
    for (int i = 0; i < PROF_POOL; i++) (void)hipEventCreate(&g_prof_ev[i]);
    g_prof_ev_ready = true;
  }
  if (g_prof_mode == 2) {
    if (g_prof_full) return;
    int base = 0;
    if (g_prof_ncalls > 0) {                 // close the previous call
      g_prof_calls[g_prof_ncalls - 1][1] = g_prof_n;
      base = g_prof_calls[g_prof_ncalls - 1][0] + g_prof_n + 1;
    }
    if (base + PROF_MAX + 1 > PROF_POOL || g_prof_ncalls >= PROF_POOL / 2) { g_prof_full = true; g_prof_n = PROF_MAX; return; }
    g_prof_base = base;
    g_prof_calls[g_prof_ncalls][0] = base;
    g_prof_calls[g_prof_ncalls][1] = 0;
    g_prof_ncalls++;
  } else {
    g_prof_base = 0;
  }
  g_prof_n = 0;
  (void)hipEventRecord(g_prof_ev[g_prof_base], stream);
}

void prof_mark(hipStream_t stream, const char* name) {
  if (!g_prof_mode || !g_prof_ev_ready || g_prof_n >= PROF_MAX || g_prof_hold) return;
  snprintf(g_prof_names[g_prof_base + g_prof_n], sizeof(g_prof_names[0]), "%s", name);
  g_prof_n++;
  (void)hipEventRecord(g_prof_ev[g_prof_base + g_prof_n], stream);
}


// RAII: while alive, the marks of the kernels a phase is made of (the transforms' passes) are dropped: the phase is one interval
struct prof_hold {
  prof_hold() { g_prof_hold = true; }
  ~prof_hold() { g_prof_hold = false; }
};

// roctx ranges, one per C-ABI call, so that `rocprofv3 --marker-trace --kernel-trace` attributes kernels to entry points (the tracing
// counterpart of the reference's per-phase `start_timer!` lines).  OPT-IN: the ranges are live when a marker library is
// ALREADY loaded in the process (a profiler brought it: found with RTLD_NOLOAD, nothing is loaded on the library's own initiative) or when
// ZKHIP_ROCTX=1 asks for it (then rocprofiler-sdk's roctx, else roctracer's, is dlopen'ed); otherwise -- every production host -- the macro
// costs one branch on a cached null pointer.  ZKHIP_NO_ROCTX=1 turns them off under a profiler too.  No link dependency either way.
struct roctx_api {
  int (*push)(const char*) = nullptr;
  int (*pop)() = nullptr;
};
static const roctx_api& roctx() {
  static const roctx_api api = [] {
    roctx_api a;
    if (getenv("ZKHIP_NO_ROCTX")) return a;
    static const char* const names[] = {"librocprofiler-sdk-roctx.so.1", "librocprofiler-sdk-roctx.so", "libroctx64.so.4", "libroctx64.so"};
    void* h = nullptr;
    for (const char* nm : names) if (!h) h = dlopen(nm, RTLD_LAZY | RTLD_LOCAL | RTLD_NOLOAD);
    const char* want = getenv("ZKHIP_ROCTX");
    if (!h && want && want[0] == '1')
      for (const char* nm : names) if (!h) h = dlopen(nm, RTLD_LAZY | RTLD_LOCAL);
    if (h) {
      a.push = (int (*)(const char*))dlsym(h, "roctxRangePushA");
      a.pop = (int (*)())dlsym(h, "roctxRangePop");
      if (!a.push || !a.pop) a.push = nullptr, a.pop = nullptr;
    }
    return a;
  }();
  return api;
}
struct api_range {
  bool on;
  explicit api_range(const char* name) : on(roctx().push != nullptr) { if (on) (void)roctx().push(name); }
  ~api_range() { if (on) (void)roctx().pop(); }
  api_range(const api_range&) = delete;
  api_range& operator=(const api_range&) = delete;
};
#define ZK_API_RANGE() zkhip::api_range zk_api_range_(__func__)

struct dev_buf {       // grow-only device scratch (hipFree waits for the device, so growing under queued work is safe)
  void* p = nullptr;
  size_t cap = 0;
  int reserve(size_t bytes) {
    if (bytes <= cap) return ZKHIP_OK;
    if (p) (void)hipFree(p);
    p = nullptr; cap = 0;
    size_t want = bytes + bytes / 8;
    if (hipMalloc(&p, want) != hipSuccess) {
      (void)hipGetLastError();
      if (hipMalloc(&p, bytes) != hipSuccess) { (void)hipGetLastError(); set_error("hipMalloc(%zu) failed", bytes); p = nullptr; return ZKHIP_ENOMEM; }
      want = bytes;
    }
    cap = want;
    return ZKHIP_OK;
  }
  void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

struct scratch {       // one user at a time: the calls of one stream
  dev_buf ws, scalars, bases, poly, poly2, small, ntt_tmp, vm, gather;
  dev_buf q_ext;                       // zkhip_fr_eval_rows_sharded_device on one device: the extended cosets of the COEFF columns
  vm_staging vm_stage;                 // pinned host staging of the row programs' blobs (rowvm.hip)
  arg_ring args;                       // pinned slots for the small host arrays of `_device` calls (lists of column addresses, coefficients)
  dev_buf transcript;                  // the transcript calls' records: a head (TR_HEAD bytes, word 0 = the call's count of identity inputs) + the payload
  int pins = 0;                        // `_device` calls that wait on this set's stream WITHOUT g_mu (the transcript's): a pinned set is not evicted
  uint64_t last_use = 0;
  // a launch of row programs on this set (rowvm.hip): the workspace reserved, the staging named; the form and the outputs are the caller's
  int vm_call_for(hipStream_t s, const zkhip_vm_program* progs, uint32_t n_progs, const void* const* d_columns, uint32_t n_columns, uint32_t log_rows, vm_call* c) {
    const int rc = vm.reserve(row_vm_workspace_bytes(progs, n_progs, n_columns, log_rows));
    if (rc != ZKHIP_OK) return rc;
    c->progs = progs; c->n_progs = n_progs; c->d_columns = d_columns; c->n_columns = n_columns; c->log_rows = log_rows;
    c->ws = vm.p; c->ws_bytes = vm.cap; c->stream = s; c->staging = &vm_stage;
    return ZKHIP_OK;
  }
  void release() { transcript.release(); ws.release(); scalars.release(); bases.release(); poly.release(); poly2.release(); small.release(); ntt_tmp.release(); vm.release(); gather.release(); q_ext.release(); vm_stage.release(); args.release(); }
};

constexpr int STREAM_PIECES_MAX = 64;      // pieces of one chunked host-buffer MSM
struct lane {          // host-buffer calls: a library-owned stream + (through the stream) a scratch set + a pinned result buffer
  hipStream_t stream = nullptr;
  void* pinned = nullptr;              // LANE_PINNED bytes, hipHostMalloc
  bool busy = false;
  // chunked host-buffer MSM (msm_shard_enqueue): the scalar pieces cross PCIe on `copy` while the pieces before them are sorted and
  // accumulated on `stream`; one event per piece in flight.  Created on first use.
  hipStream_t copy = nullptr;
  hipEvent_t copied[STREAM_PIECES_MAX] = {};
};
constexpr size_t LANE_PINNED = 64 * 1024;
constexpr size_t MAX_STREAM_SCRATCH = 8;   // scratch sets kept per device (least recently used caller streams are dropped beyond that)

// a host thread that drives one secondary device during a sharded MSM (its own PCIe link is fed by its own thread: a pageable
// hipMemcpyAsync stages through the calling thread)
struct worker {
  std::thread th;
  std::mutex mu;
  std::condition_variable cv;
  std::function<int()> job;
  bool has_job = false, done = false, quit = false;
  int rc = 0;
  char err[512] = "";
  void loop() {
    for (;;) {
      std::unique_lock<std::mutex> lk(mu);
      cv.wait(lk, [&] { return has_job || quit; });
      if (quit) return;
      std::function<int()> j = std::move(job);
      has_job = false;
      lk.unlock();
      const int r = j();
      lk.lock();
      rc = r;
      snprintf(err, sizeof(err), "%s", g_err);     // the worker thread's error text, for the caller
      done = true;
      cv.notify_all();
    }
  }
  void submit(std::function<int()> j) {
    std::lock_guard<std::mutex> lk(mu);
    job = std::move(j); has_job = true; done = false;
    cv.notify_all();
  }
  int wait() {
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { return done; });
    done = false;
    if (rc != ZKHIP_OK) set_error("%s", err);
    return rc;
  }
};

struct device_ctx {
  int device = 0;
  std::vector<lane> lanes;
  std::map<hipStream_t, scratch*> scratch_by_stream;
  uint64_t use_clock = 0;
  dev_buf fixed_table;                 // multiples of the generator for zkhip_g1_fixed_base_mul_device (primary only)
  bool fixed_table_ready = false;
  dev_buf poseidon_table;              // poseidon.hpp's table in the kernels' limbs (primary only), uploaded by the first Poseidon `_device` call
  bool poseidon_table_ready = false;
  dev_buf gather;                      // primary: the shards' 96-byte partials, one 96-byte slot per shard
  std::vector<hipEvent_t> shard_events;
  hipStream_t side = nullptr;          // primary: second stream of a batch of large MSMs (high priority: never the caller's hardware queue)
  hipEvent_t side_fork = nullptr, side_join = nullptr;
  worker* w = nullptr;                 // secondary devices only
  // multi-device `_device` calls (fan_call below, their only user): a secondary device runs its share on `fan`, a stream of its own (not the
  // lane its worker thread drives for host-buffer calls), behind `fan_ready` of the primary device (recorded on the caller's stream: the
  // inputs are complete) and records `fan_done` for the caller's stream to wait on
  hipStream_t fan = nullptr;
  hipEvent_t fan_ready = nullptr, fan_done = nullptr;
  // the sharded quotient numerator (zkhip_fr_eval_rows_sharded_device): the extended cosets of the COEFF columns this device owns, its window
  // buffers and (secondaries) its rows' results; `q_transformed` follows its transforms, `q_done` its last step (the next call's first steps wait on it)
  dev_buf q_ext, q_win, q_out;
  hipEvent_t q_transformed = nullptr, q_done = nullptr;
  bool q_done_live = false;
};

struct shard_t {       // points [lo, lo + n) of a registered array, prepared on device `dev`
  int dev = 0;         // index into g_ctx.devs
  size_t lo = 0, n = 0;
  prepared_bases* pb = nullptr;
};

constexpr int FINGER_POINTS = 8;
struct registered_t {  // one zkhip_register_bases call
  const uint64_t* host = nullptr;
  size_t n = 0;
  std::vector<shard_t> shards;
  size_t finger_idx[FINGER_POINTS];
  uint64_t finger[FINGER_POINTS][8];   // sampled points of the host array at registration: a stale or modified range is not trusted
  ~registered_t();
};

// A row-shard set (zkhip_row_shards_create): n_cols columns of a 2^ext_k domain cut by rows over the S devices of zkhip_init, device j holding
// [col][W_j] window buffers (W_j = halo_lo + count_j + halo_hi) in one allocation.  `last` keeps, per device, one event per stream that has
// enqueued work on the set: destroy waits for those, not for the devices.
struct row_shards_t {
  uint32_t ext_k = 0, n_cols = 0;
  uint64_t halo_lo = 0, halo_hi = 0;
  int S = 0;
  std::vector<void*> mem;
  std::vector<uint64_t> row0, count;
  std::vector<std::map<hipStream_t, hipEvent_t>> last;
  uint64_t W(int j) const { return halo_lo + count[(size_t)j] + halo_hi; }
  uint32_t* window(int j, uint32_t col) const { return (uint32_t*)mem[(size_t)j] + (size_t)col * W(j) * 8; }
};

struct context {
  bool ready = false;
  std::vector<device_ctx*> devs;       // devs[0] = primary
  int shards = 1;                      // MSM shards a registered array is cut into (default: one per device)
  int ntt_fanout = 1;                  // batched transforms over the devices: 0 never, 1 host-buffer forms, 2 `_device` forms too (zkhip_set_ntt_fanout)
  std::map<const void*, std::shared_ptr<registered_t>> registered;
  std::map<uint64_t, prepared_bases*> handles;          // zkhip_prepare_bases_device handles (primary device)
  uint64_t next_handle = 1;
  std::map<uintptr_t, row_shards_t*> sets;              // live row-shard sets by handle (handles are never reused)
  uintptr_t next_set = 0x10;
};

static std::recursive_mutex g_mu;
static std::condition_variable_any g_lane_cv;
static std::mutex g_fanout_mu;         // one multi-device MSM at a time (the secondary devices have one lane each)
static context g_ctx;

static inline device_ctx& primary() { return *g_ctx.devs[0]; }

registered_t::~registered_t() {
  for (auto& sh : shards) {
    if (!sh.pb) continue;
    if (g_ctx.ready && sh.dev < (int)g_ctx.devs.size()) (void)hipSetDevice(g_ctx.devs[sh.dev]->device);
    release_prepared(sh.pb);
  }
  if (g_ctx.ready) (void)hipSetDevice(primary().device);
}

static int ensure_init() {
  if (!g_ctx.ready) return zkhip_init(nullptr, 0);
  // the current device is per host thread: a rayon worker that never touched HIP starts on device 0
  int cur = -1;
  if (hipGetDevice(&cur) != hipSuccess || cur != primary().device) {
    if (hipSetDevice(primary().device) != hipSuccess) { set_error("hipSetDevice(%d) failed", primary().device); return ZKHIP_ENODEV; }
  }
  return ZKHIP_OK;
}

// scratch set of `stream` on device d (g_mu held).  Beyond MAX_STREAM_SCRATCH sets the least recently used one that does not belong
// to a library lane is dropped (after a device synchronisation: its stream may have been destroyed by the caller).
static scratch* scratch_for(device_ctx& d, hipStream_t stream) {
  auto it = d.scratch_by_stream.find(stream);
  if (it != d.scratch_by_stream.end()) { it->second->last_use = ++d.use_clock; return it->second; }
  if (d.scratch_by_stream.size() >= MAX_STREAM_SCRATCH + d.lanes.size()) {
    auto victim = d.scratch_by_stream.end();
    for (auto jt = d.scratch_by_stream.begin(); jt != d.scratch_by_stream.end(); ++jt) {
      bool is_lane = (jt->first == d.side && d.side != nullptr) || (jt->first == d.fan && d.fan != nullptr);
      for (auto& L : d.lanes) is_lane |= (L.stream == jt->first);
      if (is_lane || jt->second->pins) continue;
      if (victim == d.scratch_by_stream.end() || jt->second->last_use < victim->second->last_use) victim = jt;
    }
    if (victim != d.scratch_by_stream.end()) {
      (void)hipDeviceSynchronize();
      victim->second->release();
      delete victim->second;
      d.scratch_by_stream.erase(victim);
    }
  }
  scratch* sc = new scratch();
  sc->last_use = ++d.use_clock;
  d.scratch_by_stream[stream] = sc;
  return sc;
}

// `stream` argument of the `_device` entry points: NULL is HIP's default (legacy) stream -- stream 0, which is what a caller
// holding "the default stream" (e.g. torch.cuda.current_stream().cuda_stream == 0) passes, and which is ordered with that caller's
// other default-stream work.
static inline hipStream_t caller_stream(void* stream) { return (hipStream_t)stream; }

// ---- lanes -----------------------------------------------------------------------------------------------------------
// RAII: one user's turn on a lane, with the lane's stream and scratch set resolved.  Construct WITHOUT holding g_mu.
// The rule for work on a lane: a call gives the lane up with nothing of its own still queued.  A call that succeeds ends in
// finish(), its one wait for the stream.  A hold that goes away without it -- any error return after the first enqueue -- waits in its destructor for
// the lane's stream and copy stream first: the caller's buffers may be pinned memory that an upload is still reading, and the lane's scratch goes to
// the next user.
struct lane_hold {
  lane* L = nullptr;
  scratch* sc = nullptr;
  hipStream_t s = nullptr;
  int rc = ZKHIP_OK;
  bool borrowed = false, clean = false;
  lane_hold() {                        // borrows a free lane of the primary device (waits for one)
    std::unique_lock<std::recursive_mutex> lk(g_mu);
    rc = ensure_init();
    if (rc != ZKHIP_OK) return;
    for (;;) {
      for (auto& c : primary().lanes) if (!c.busy) { L = &c; break; }
      if (L) break;
      g_lane_cv.wait(lk);
      if (!g_ctx.ready) { rc = ZKHIP_ENODEV; set_error("library shut down while a call was waiting"); return; }
    }
    L->busy = borrowed = true;
    s = L->stream;
    sc = scratch_for(primary(), s);
  }
  explicit lane_hold(device_ctx& D) : L(&D.lanes[0]), s(D.lanes[0].stream) {   // the one lane of a secondary device (its users take turns under g_fanout_mu)
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    sc = scratch_for(D, s);
  }
  int finish() {
    HIPCHK(hipStreamSynchronize(s));
    clean = true;
    return ZKHIP_OK;
  }
  void reopen() { clean = false; }     // a call of several rounds (chunks, vectors of a batch) enqueues again after a finish()
  ~lane_hold() {
    if (!L) return;
    if (!clean) {
      (void)hipStreamSynchronize(s);
      if (L->copy) (void)hipStreamSynchronize(L->copy);
      (void)hipGetLastError();
    }
    if (!borrowed) return;
    std::lock_guard<std::recursive_mutex> lk(g_mu);
    L->busy = false;
    g_lane_cv.notify_one();
  }
  lane_hold(const lane_hold&) = delete;
  lane_hold& operator=(const lane_hold&) = delete;
};

// Contiguous point range of shard s of S over n points: the first n % S shards get one extra point (the partition the multi-process
// path uses too: zksnap_circuits_halo2_amd/multi_gpu.py shard_range)
static inline void shard_range(size_t n, int s, int S, size_t* lo, size_t* hi) {
  const size_t base = n / (size_t)S, extra = n % (size_t)S;
  *lo = (size_t)s * base + std::min<size_t>((size_t)s, extra);
  *hi = *lo + base + ((size_t)s < extra ? 1 : 0);
}

// registered entry + point offset for `bases` if it lies inside a registered range with room for n points and the sampled points
// of that range still hold what was registered (g_mu held)
static std::shared_ptr<registered_t> find_registered(const uint64_t* bases, size_t n, size_t* off) {
  for (auto& kv : g_ctx.registered) {
    const char* lo = (const char*)kv.first;
    const char* hi = lo + kv.second->n * 64;
    const char* q = (const char*)bases;
    if (q >= lo && q + n * 64 <= hi && ((q - lo) % 64) == 0) {
      const registered_t& r = *kv.second;
      for (int i = 0; i < FINGER_POINTS; i++)
        if (memcmp(r.host + r.finger_idx[i] * 8, r.finger[i], 64) != 0) return nullptr;   // reused or modified memory: not the registered SRS
      *off = (size_t)(q - lo) / 64;
      return kv.second;
    }
  }
  return nullptr;
}

static void destroy_device_ctx(device_ctx* d) {
  (void)hipSetDevice(d->device);
  (void)hipDeviceSynchronize();
  if (d->w) {
    { std::lock_guard<std::mutex> lk(d->w->mu); d->w->quit = true; d->w->cv.notify_all(); }
    if (d->w->th.joinable()) d->w->th.join();
    delete d->w;
  }
  for (auto& kv : d->scratch_by_stream) { kv.second->release(); delete kv.second; }
  d->scratch_by_stream.clear();
  for (auto& L : d->lanes) {
    if (L.pinned) (void)hipHostFree(L.pinned);
    if (L.stream) (void)hipStreamDestroy(L.stream);
    if (L.copy) (void)hipStreamDestroy(L.copy);
    for (auto& e : L.copied) if (e) (void)hipEventDestroy(e);
  }
  for (auto e : d->shard_events) (void)hipEventDestroy(e);
  if (d->side_fork) (void)hipEventDestroy(d->side_fork);
  if (d->side_join) (void)hipEventDestroy(d->side_join);
  if (d->side) (void)hipStreamDestroy(d->side);
  if (d->fan_ready) (void)hipEventDestroy(d->fan_ready);
  if (d->fan_done) (void)hipEventDestroy(d->fan_done);
  if (d->fan) (void)hipStreamDestroy(d->fan);
  if (d->q_transformed) (void)hipEventDestroy(d->q_transformed);
  if (d->q_done) (void)hipEventDestroy(d->q_done);
  d->q_ext.release(); d->q_win.release(); d->q_out.release();
  d->fixed_table.release();
  d->poseidon_table.release();
  d->gather.release();
  delete d;
}

// ---- row-shard sets (g_mu held) ----------------------------------------------------------------------------------------
static void wait_row_shards(row_shards_t* R) {
  for (size_t j = 0; j < R->last.size() && j < g_ctx.devs.size(); j++) {
    (void)hipSetDevice(g_ctx.devs[j]->device);
    for (auto& kv : R->last[j]) (void)hipEventSynchronize(kv.second);
  }
  if (!g_ctx.devs.empty()) (void)hipSetDevice(primary().device);
}

static void free_row_shards(row_shards_t* R) {
  wait_row_shards(R);
  for (size_t j = 0; j < R->mem.size(); j++) {
    if (j < g_ctx.devs.size()) (void)hipSetDevice(g_ctx.devs[j]->device);
    for (auto& kv : R->last[j]) (void)hipEventDestroy(kv.second);
    if (R->mem[j]) (void)hipFree(R->mem[j]);
  }
  if (!g_ctx.devs.empty()) (void)hipSetDevice(primary().device);
  (void)hipGetLastError();
  delete R;
}

// the live set behind a handle, made under the current device count (else ZKHIP_EINVAL with a message, nothing touched)
static row_shards_t* find_row_shards(const zkhip_row_shards* h, const char* who) {
  auto it = g_ctx.sets.find((uintptr_t)h);
  if (!h || it == g_ctx.sets.end()) { set_error("%s: not a live row-shard set (destroyed, freed by zkhip_shutdown, or never issued)", who); return nullptr; }
  if (it->second->S != (int)g_ctx.devs.size()) { set_error("%s: set made over %d devices, zkhip_init has %zu", who, it->second->S, g_ctx.devs.size()); return nullptr; }
  return it->second;
}

// device j is current; the set's event for `st` on device j follows the work just enqueued there
static int touch_row_shards(row_shards_t* R, int j, hipStream_t st) {
  auto& m = R->last[(size_t)j];
  auto it = m.find(st);
  if (it == m.end()) {
    hipEvent_t e = nullptr;
    HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    it = m.emplace(st, e).first;
  }
  HIPCHK(hipEventRecord(it->second, st));
  return ZKHIP_OK;
}

// window pieces: dst[t] = src[(start + t) mod N] for t < W, as at most ceil(W / N) + 1 copies on `st`
static int copy_window(uint32_t* dst, int dst_dev, const uint32_t* src, int src_dev, size_t start, size_t W, size_t N, hipStream_t st) {
  for (size_t t = 0, pos = start; t < W;) {
    const size_t len = std::min(W - t, N - pos);
    HIPCHK(hipMemcpyPeerAsync(dst + t * 8, dst_dev, src + pos * 8, src_dev, len * 32, st));
    t += len;
    pos = 0;
  }
  return ZKHIP_OK;
}

static inline size_t window_start(uint64_t row0, uint64_t halo_lo, size_t N) {
  return (size_t)((((int64_t)row0 - (int64_t)halo_lo) % (int64_t)N + (int64_t)N) % (int64_t)N);
}

// One multi-device `_device` call (g_mu held by the caller): `begin` records the entry event on the caller's stream s; dev(j) makes device j current and, the first time, gives it its stream st[j] -- s on the primary, elsewhere the device's fan
// stream behind the entry event (a device the call never names gets no work); `end` makes s wait for every secondary that was named.
// The rule for work on these streams is the lanes' (DESIGN.md section 8): a call that does not reach `end` -- any error return after `begin` -- waits
// in the destructor for every stream it named, so that nothing of it outlives the call's buffers.
struct fan_call {
  std::vector<hipStream_t> st;         // st[j] is null until dev(j)
  hipStream_t s = nullptr;
  bool armed = true;
  int begin(hipStream_t caller) {
    s = caller;
    st.assign(g_ctx.devs.size(), nullptr);
    if (st.size() == 1) return ZKHIP_OK;
    device_ctx& P = primary();
    if (!P.fan_ready) HIPCHK(hipEventCreateWithFlags(&P.fan_ready, hipEventDisableTiming));
    HIPCHK(hipEventRecord(P.fan_ready, s));
    return ZKHIP_OK;
  }
  int dev(int j) {
    device_ctx* D = g_ctx.devs[(size_t)j];
    if (hipSetDevice(D->device) != hipSuccess) { set_error("hipSetDevice(%d) failed", D->device); return ZKHIP_ENODEV; }
    if (st[(size_t)j]) return ZKHIP_OK;
    if (j == 0) { st[0] = s; return ZKHIP_OK; }
    if (!D->fan) {
      HIPCHK(hipStreamCreateWithFlags(&D->fan, hipStreamNonBlocking));
      HIPCHK(hipEventCreateWithFlags(&D->fan_done, hipEventDisableTiming));
    }
    st[(size_t)j] = D->fan;
    HIPCHK(hipStreamWaitEvent(D->fan, primary().fan_ready, 0));
    return ZKHIP_OK;
  }
  int end() {
    for (size_t j = 1; j < st.size(); j++) {
      if (!st[j]) continue;
      device_ctx* D = g_ctx.devs[j];
      if (hipSetDevice(D->device) != hipSuccess) { set_error("hipSetDevice(%d) failed", D->device); return ZKHIP_ENODEV; }
      HIPCHK(hipEventRecord(D->fan_done, D->fan));
    }
    if (hipSetDevice(primary().device) != hipSuccess) { set_error("hipSetDevice(%d) failed", primary().device); return ZKHIP_ENODEV; }
    for (size_t j = 1; j < st.size(); j++)
      if (st[j]) HIPCHK(hipStreamWaitEvent(s, g_ctx.devs[j]->fan_done, 0));
    armed = false;
    return ZKHIP_OK;
  }
  ~fan_call() {
    if (!armed) return;
    for (size_t j = 0; j < st.size(); j++)
      if (st[j]) { (void)hipSetDevice(g_ctx.devs[j]->device); (void)hipStreamSynchronize(st[j]); }
    if (!g_ctx.devs.empty()) (void)hipSetDevice(primary().device);
    (void)hipGetLastError();
  }
};

}  // namespace zkhip

using namespace zkhip;
typedef std::lock_guard<std::recursive_mutex> guard_t;

extern "C" {

int zkhip_init(const int* devices, int ndev) {
  ZK_API_RANGE();
  guard_t g(g_mu);
  if (ndev < 0 || ndev > 64) { set_error("zkhip_init: ndev = %d out of range", ndev); return ZKHIP_EINVAL; }
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count == 0) { (void)hipGetLastError(); set_error("no HIP device available"); return ZKHIP_ENODEV; }
  std::vector<int> want;
  if (devices && ndev >= 1) want.assign(devices, devices + ndev);
  else if (const char* e = getenv("ZKHIP_DEVICE")) want.push_back(atoi(e));
  else want.push_back(0);
  for (size_t i = 0; i < want.size(); i++) {
    if (want[i] < 0 || want[i] >= count) { set_error("device %d out of range (%d devices)", want[i], count); return ZKHIP_EINVAL; }
    // a device named twice is an error -- except under ZKHIP_TEST_DUPLICATE_DEVICES=1, which lets a one-GPU box rehearse the
    // multi-device machinery (worker threads, peer copies, gather + fold) with several contexts on the same card
    const bool dup_ok = getenv("ZKHIP_TEST_DUPLICATE_DEVICES") != nullptr;
    for (size_t j = 0; j < i && !dup_ok; j++) if (want[j] == want[i]) { set_error("zkhip_init: device %d named twice", want[i]); return ZKHIP_EINVAL; }
  }
  if (g_ctx.ready) {
    bool same = g_ctx.devs.size() == want.size();
    for (size_t i = 0; same && i < want.size(); i++) same = g_ctx.devs[i]->device == want[i];
    if (same) return ensure_init();
    // a host-buffer call in flight holds a lane without the lock; shutdown would wait for it on a mutex this thread holds twice
    // (condition_variable_any releases one level only): refuse instead of deadlocking
    for (auto& L : primary().lanes) if (L.busy) { set_error("zkhip_init: a different device list while host-buffer calls are in flight"); return ZKHIP_EBUSY; }
    zkhip_shutdown();
  }
  int lanes = 2;                                            // host-buffer calls that may be in flight at once
  if (const char* e = getenv("ZKHIP_HOST_LANES")) { const int v = atoi(e); if (v >= 1 && v <= 4) lanes = v; }
  for (size_t i = 0; i < want.size(); i++) {
    if (hipSetDevice(want[i]) != hipSuccess) { (void)hipGetLastError(); set_error("hipSetDevice(%d) failed", want[i]); for (auto d : g_ctx.devs) destroy_device_ctx(d); g_ctx.devs.clear(); return ZKHIP_ENODEV; }
    device_ctx* d = new device_ctx();
    d->device = want[i];
    d->lanes.resize(i == 0 ? (size_t)lanes : 1);
    bool ok = true;
    for (auto& L : d->lanes) {
      ok = ok && hipStreamCreateWithFlags(&L.stream, hipStreamNonBlocking) == hipSuccess;
      ok = ok && hipHostMalloc(&L.pinned, LANE_PINNED, hipHostMallocDefault) == hipSuccess;
    }
    g_ctx.devs.push_back(d);
    if (!ok) { (void)hipGetLastError(); set_error("zkhip_init: stream / pinned buffer creation failed on device %d", want[i]); for (auto dd : g_ctx.devs) destroy_device_ctx(dd); g_ctx.devs.clear(); return ZKHIP_ENODEV; }
    if (i > 0) {
      d->w = new worker();
      const int devno = want[i];
      worker* w = d->w;
      w->th = std::thread([w, devno] { (void)hipSetDevice(devno); w->loop(); });
    }
  }
  // partial sums travel device to device (xGMI); without peer access hipMemcpyPeerAsync stages through the host, which is also fine
  for (size_t i = 1; i < want.size(); i++) {
    int can = 0;
    if (hipDeviceCanAccessPeer(&can, want[i], want[0]) == hipSuccess && can) {
      (void)hipSetDevice(want[i]);
      (void)hipDeviceEnablePeerAccess(want[0], 0);
    }
    (void)hipGetLastError();
  }
  (void)hipSetDevice(want[0]);
  g_ctx.shards = (int)want.size();
  if (const char* e = getenv("ZKHIP_SHARDS")) { const int v = atoi(e); if (v >= 1 && v <= 64) g_ctx.shards = v; }
  g_ctx.ntt_fanout = 1;
  if (const char* e = getenv("ZKHIP_NTT_FANOUT")) { const int v = atoi(e); if (v >= 0 && v <= 2) g_ctx.ntt_fanout = v; }
  g_ctx.ready = true;
  return ZKHIP_OK;
}

void zkhip_shutdown(void) {
  ZK_API_RANGE();
  std::unique_lock<std::recursive_mutex> lk(g_mu);
  if (!g_ctx.ready) return;
  // host-buffer calls in flight hold a lane without the lock: let them finish
  for (;;) {
    bool busy = false;
    for (auto& L : primary().lanes) busy |= L.busy;
    for (auto& kv : primary().scratch_by_stream) busy |= kv.second->pins != 0;      // a transcript `_device` call is waiting on its stream
    if (!busy) break;
    g_lane_cv.wait(lk);
  }
  (void)hipSetDevice(primary().device);
  (void)hipDeviceSynchronize();
  ntt_clear_cache();
  row_vm_jit_clear();
  g_ctx.registered.clear();                                  // last references: tables are freed by ~registered_t
  for (auto& kv : g_ctx.handles) release_prepared(kv.second);
  g_ctx.handles.clear();
  for (auto& kv : g_ctx.sets) free_row_shards(kv.second);
  g_ctx.sets.clear();
  for (auto d : g_ctx.devs) destroy_device_ctx(d);
  g_ctx.devs.clear();
  g_ctx.ready = false;
  g_lane_cv.notify_all();
}

const char* zkhip_last_error(void) { return g_err; }

int zkhip_device_name(char* buf, size_t len) {
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, primary().device));
  snprintf(buf, len, "%s (%s, %d CUs)", prop.name, prop.gcnArchName, prop.multiProcessorCount);
  return ZKHIP_OK;
}

int zkhip_device_count(void) {
  guard_t g(g_mu);
  if (ensure_init() != ZKHIP_OK) return 0;
  return (int)g_ctx.devs.size();
}

int zkhip_set_msm_shards(int shards) {
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  if (shards < 0 || shards > 64) { set_error("set_msm_shards: %d out of range [0, 64]", shards); return ZKHIP_EINVAL; }
  g_ctx.shards = shards == 0 ? (int)g_ctx.devs.size() : shards;
  return ZKHIP_OK;
}

int zkhip_msm_shards(void) {
  guard_t g(g_mu);
  if (ensure_init() != ZKHIP_OK) return 0;
  return g_ctx.shards;
}

int zkhip_msm_window_bits(size_t n) { return msm_pick_window(n); }

// ---- MSM -----------------------------------------------------------------------------------------
int zkhip_msm_g1_device_c(const void* d_scalars, const void* d_bases, size_t n, void* d_out_xyz, int window_bits, void* stream) {
  ZK_API_RANGE();
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  if (!d_out_xyz || (n && (!d_scalars || !d_bases))) { set_error("msm: null pointer"); return ZKHIP_EINVAL; }
  const int c = window_bits > 0 ? window_bits : msm_pick_window(n ? n : 1);
  hipStream_t s = caller_stream(stream);
  scratch* sc = scratch_for(primary(), s);
  if ((rc = sc->ws.reserve(msm_workspace_bytes(n, c))) != ZKHIP_OK) return rc;
  return msm_g1_device((const uint32_t*)d_scalars, (const uint32_t*)d_bases, n, (uint32_t*)d_out_xyz, sc->ws.p, sc->ws.cap, c, s);
}

int zkhip_msm_g1_device(const void* d_scalars, const void* d_bases, size_t n, void* d_out_xyz, void* stream) {
  ZK_API_RANGE();
  return zkhip_msm_g1_device_c(d_scalars, d_bases, n, d_out_xyz, 0, stream);
}

}  // extern "C"

namespace zkhip {

// One shard's share of a host-buffer MSM on the held lane U (its device is the current one): uploads the scalar slice (and the base slice
// when there is no prepared table), runs the MSM, leaves the 96-byte partial at d_partial (memory of that device).
// Chunked upload (round 4).  A host-buffer MSM used to upload all its scalars with one copy and only then start its first kernel (2^22 points:
// 2.4 ms of PCIe + 4.9 ms of kernels, nothing overlapped).  With a prepared table of wide windows and at least two pieces of 2^20 scalars the
// upload is cut into J even pieces on the lane's copy stream; piece j is sorted and accumulated into the shared bucket set (msm.hip:
// msm_chunk_add) while piece j + 1 crosses PCIe, and one reduction tail ends the call.  Only the first piece's upload is exposed.
// ZKHIP_STREAM_PIECE_LOG: log2 of the target piece size (default 20; 0 = never chunk).
static size_t msm_stream_pieces(size_t n, const prepared_bases* pb) {
  static const int piece_log = [] { const char* e = getenv("ZKHIP_STREAM_PIECE_LOG"); const int v = e ? atoi(e) : 20; return (v == 0 || (v >= 16 && v <= 26)) ? v : 20; }();
  if (!pb || pb->c <= 16 || piece_log == 0) return 1;
  const size_t J = n >> piece_log;
  return J < 2 ? 1 : std::min<size_t>(J, (size_t)STREAM_PIECES_MAX);
}

static int msm_shard_enqueue_chunked(lane_hold& U, const uint64_t* scalars, size_t n, const prepared_bases* pb, size_t pb_off, uint32_t* d_partial, size_t J,
                                     size_t region) {
  int rc;
  lane* const L = U.L;
  scratch* const sc = U.sc;
  hipStream_t s = U.s;
  if (!L->copy) HIPCHK(hipStreamCreateWithFlags(&L->copy, hipStreamNonBlocking));
  const size_t cap = (n + J - 1) / J;
  const size_t ws_bytes = msm_chunk_workspace_bytes(cap, pb->c);
  if ((rc = sc->scalars.reserve((region + n) * 32)) != ZKHIP_OK) return rc;      // (a no-op inside a fan-out: reserve_for_pieces sized the buffer for all pieces)
  if ((rc = sc->ws.reserve(ws_bytes)) != ZKHIP_OK) return rc;
  // (a non-OK exit below leaves pieces crossing PCIe from the caller's buffer on the copy stream: the hold waits for that stream too)
  // Every piece of a call has its own region of the lane's scalar buffer (`region`, in scalars), so the copy stream may run ahead of the kernels:
  // while shard k is being accumulated on `s`, the pieces of shard k + 1 are already crossing PCIe (virtual shards on one lane).  A call ends with
  // hipStreamSynchronize(s), and `s` waits for every copy it used, so nothing of an earlier call is in flight here.
  char* const dst = (char*)sc->scalars.p + region * 32;
  size_t lo = 0;
  for (size_t j = 0; j < J; j++) {
    const size_t len = n / J + (j < n % J ? 1 : 0);          // cap or cap - 1
    if (!L->copied[j]) HIPCHK(hipEventCreateWithFlags(&L->copied[j], hipEventDisableTiming));
    HIPCHK(hipMemcpyAsync(dst + lo * 32, scalars + lo * 4, len * 32, hipMemcpyHostToDevice, L->copy));
    HIPCHK(hipEventRecord(L->copied[j], L->copy));
    HIPCHK(hipStreamWaitEvent(s, L->copied[j], 0));
    if ((rc = msm_chunk_add((const uint32_t*)(dst + lo * 32), len, pb, pb_off + lo, cap, j == 0, sc->ws.p, sc->ws.cap, s)) != ZKHIP_OK) return rc;
    lo += len;
  }
  return msm_chunk_finish(pb, cap, d_partial, sc->ws.p, sc->ws.cap, s);
}

// region: offset (in scalars) of this piece inside the lane's scalar buffer -- the pieces one lane runs back to back (virtual shards) do not share
// upload space, so one piece's upload never waits for the previous piece's kernels
static int msm_shard_enqueue(lane_hold& U, const uint64_t* scalars, const uint64_t* bases, size_t n, const prepared_bases* pb, size_t pb_off, uint32_t* d_partial,
                             size_t region = 0) {
  int rc;
  scratch* const sc = U.sc;
  hipStream_t s = U.s;
  if (n == 0) return msm_g1_device(nullptr, nullptr, 0, d_partial, nullptr, 0, 0, s);
  const size_t J = msm_stream_pieces(n, pb);
  if (J > 1) return msm_shard_enqueue_chunked(U, scalars, n, pb, pb_off, d_partial, J, region);
  if ((rc = sc->scalars.reserve((region + n) * 32)) != ZKHIP_OK) return rc;
  char* const d_sc = (char*)sc->scalars.p + region * 32;
  HIPCHK(hipMemcpyAsync(d_sc, scalars, n * 32, hipMemcpyHostToDevice, s));
  if (pb) {
    if ((rc = sc->ws.reserve(msm_workspace_bytes(n, pb->c, true))) != ZKHIP_OK) return rc;
    return msm_g1_device((const uint32_t*)d_sc, nullptr, n, d_partial, sc->ws.p, sc->ws.cap, 0, s, pb, pb_off);
  }
  if ((rc = sc->bases.reserve(n * 64)) != ZKHIP_OK) return rc;
  HIPCHK(hipMemcpyAsync(sc->bases.p, bases, n * 64, hipMemcpyHostToDevice, s));
  const int c = msm_pick_window(n);
  if ((rc = sc->ws.reserve(msm_workspace_bytes(n, c))) != ZKHIP_OK) return rc;
  return msm_g1_device((const uint32_t*)d_sc, (const uint32_t*)sc->bases.p, n, d_partial, sc->ws.p, sc->ws.cap, c, s);
}

struct piece_t { int dev; size_t lo, n; const prepared_bases* pb; size_t pb_off; };   // points [lo, lo + n) of the call's range

// Size the scratch for the pieces one device will run back to back (scalars: the sum, one region per piece; bases and workspace: the largest):
// growing a buffer between two pieces would free it (a device-wide wait) under the previous piece's kernels.
static int reserve_for_pieces(scratch* sc, const std::vector<piece_t>& pieces, const std::vector<size_t>& mine) {
  size_t sc_bytes = 0, bs_bytes = 0, ws_bytes = 0;
  for (size_t i : mine) {
    const piece_t& p = pieces[i];
    if (p.n == 0) continue;
    sc_bytes += p.n * 32;                           // one region per piece (msm_shard_enqueue)
    if (!p.pb) bs_bytes = std::max(bs_bytes, p.n * 64);
    const size_t J = msm_stream_pieces(p.n, p.pb);
    if (J > 1) ws_bytes = std::max(ws_bytes, msm_chunk_workspace_bytes((p.n + J - 1) / J, p.pb->c));
    else ws_bytes = std::max(ws_bytes, p.pb ? msm_workspace_bytes(p.n, p.pb->c, true) : msm_workspace_bytes(p.n, msm_pick_window(p.n)));
  }
  int rc;
  if ((rc = sc->scalars.reserve(sc_bytes)) != ZKHIP_OK) return rc;
  if ((rc = sc->bases.reserve(bs_bytes)) != ZKHIP_OK) return rc;
  return sc->ws.reserve(ws_bytes);
}

// Host-buffer MSM on a borrowed lane: out = sum scalars[i] * bases[i].  `reg` (may be null) = the registered entry `bases` points
// into at point offset `off`.  Pieces = the shards the range touches (registered) or an even split over the devices (not registered,
// several devices); a single piece on the primary device is the plain path.
static int host_msm(lane_hold& H, const uint64_t* scalars, const uint64_t* bases, size_t n, const std::shared_ptr<registered_t>& reg, size_t off,
                    uint64_t* out_xyz) {
  int rc;
  H.reopen();                                           // (zkhip_msm_g1_batch runs its vectors through here one after the other)
  std::vector<piece_t> pieces;
  if (reg) {
    for (auto& sh : reg->shards) {
      const size_t lo = std::max(off, sh.lo), hi = std::min(off + n, sh.lo + sh.n);
      if (lo < hi) pieces.push_back({sh.dev, lo - off, hi - lo, sh.pb, lo - sh.lo});
    }
  } else if (g_ctx.devs.size() > 1 && n >= 4096 * g_ctx.devs.size()) {
    const int S = (int)g_ctx.devs.size();
    for (int s = 0; s < S; s++) {
      size_t lo, hi;
      shard_range(n, s, S, &lo, &hi);
      if (lo < hi) pieces.push_back({s, lo, hi - lo, nullptr, 0});
    }
  }
  if (pieces.empty()) pieces.push_back({0, 0, n, nullptr, 0});
  hipStream_t s = H.s;
  scratch* sc = H.sc;
  if ((rc = sc->small.reserve(4096)) != ZKHIP_OK) return rc;
  if (pieces.size() == 1 && pieces[0].dev == 0) {
    const piece_t& p = pieces[0];
    if ((rc = msm_shard_enqueue(H, scalars + p.lo * 4, bases + p.lo * 8, p.n, p.pb, p.pb_off, (uint32_t*)sc->small.p)) != ZKHIP_OK) return rc;
  } else {
    // fan out: the primary device's pieces run on this thread's lane, one after another (virtual shards) -- the other devices'
    // pieces on their worker threads, each device over its own PCIe link
    device_ctx& P = primary();
    std::unique_lock<std::mutex> fan(g_fanout_mu, std::defer_lock);
    bool remote = false;
    for (auto& p : pieces) remote |= p.dev != 0;
    if (remote) fan.lock();
    // gather slots live in the lane's scratch set: concurrent single-device fan-outs on different lanes do not share them
    if ((rc = sc->poly2.reserve(pieces.size() * 96 + 256)) != ZKHIP_OK) return rc;
    uint32_t* gather = (uint32_t*)sc->poly2.p;
    std::vector<std::vector<size_t>> by_dev(g_ctx.devs.size());
    for (size_t i = 0; i < pieces.size(); i++) by_dev[(size_t)pieces[i].dev].push_back(i);
    if ((rc = reserve_for_pieces(sc, pieces, by_dev[0])) != ZKHIP_OK) return rc;
    for (size_t d = 1; d < g_ctx.devs.size(); d++) {
      if (by_dev[d].empty()) continue;
      device_ctx* D = g_ctx.devs[d];
      const std::vector<size_t> mine = by_dev[d];
      const int primary_dev = P.device;
      D->w->submit([D, mine, &pieces, scalars, bases, gather, primary_dev]() -> int {
        lane_hold U(*D);                                  // a failed job has drained the lane before wait() hands its error to the caller
        scratch* dsc = U.sc;
        int r;
        if ((r = dsc->small.reserve(4096 + mine.size() * 96)) != ZKHIP_OK) return r;
        if ((r = reserve_for_pieces(dsc, pieces, mine)) != ZKHIP_OK) return r;
        size_t region = 0;
        for (size_t k = 0; k < mine.size(); k++) {
          const piece_t& p = pieces[mine[k]];
          uint32_t* part = (uint32_t*)((char*)dsc->small.p + 4096 + k * 96);
          if ((r = msm_shard_enqueue(U, scalars + p.lo * 4, bases + p.lo * 8, p.n, p.pb, p.pb_off, part, region)) != ZKHIP_OK) return r;
          region += p.n;
          HIPCHK(hipMemcpyPeerAsync(gather + mine[k] * 24, primary_dev, part, D->device, 96, U.s));
        }
        return U.finish();                                // the partials have landed on the primary device
      });
    }
    int rc_local = ZKHIP_OK;
    size_t region0 = 0;
    for (size_t i : by_dev[0]) {
      const piece_t& p = pieces[i];
      if ((rc_local = msm_shard_enqueue(H, scalars + p.lo * 4, bases + p.lo * 8, p.n, p.pb, p.pb_off, gather + i * 24, region0)) != ZKHIP_OK) break;
      region0 += p.n;
    }
    int rc_remote = ZKHIP_OK;
    for (size_t d = 1; d < g_ctx.devs.size(); d++) {
      if (by_dev[d].empty()) continue;
      const int r = g_ctx.devs[d]->w->wait();
      if (r != ZKHIP_OK) rc_remote = r;
    }
    if (rc_local != ZKHIP_OK) return rc_local;
    if (rc_remote != ZKHIP_OK) return rc_remote;
    // the remote partials were written by other devices' streams, which this thread has waited for; the fold is ordered behind
    // the local pieces on the lane's stream
    if ((rc = sum_jacobian_device(gather, (int)pieces.size(), (uint32_t*)sc->small.p, s)) != ZKHIP_OK) return rc;
  }
  HIPCHK(hipMemcpyAsync(H.L->pinned, sc->small.p, 96, hipMemcpyDeviceToHost, s));
  if ((rc = H.finish()) != ZKHIP_OK) return rc;
  memcpy(out_xyz, H.L->pinned, 96);
  return ZKHIP_OK;
}

}  // namespace zkhip

extern "C" {

int zkhip_msm_g1(const uint64_t* scalars, const uint64_t* bases, size_t n, uint64_t out_xyz[12]) {
  ZK_API_RANGE();
  if (!out_xyz || (n && (!scalars || !bases))) { set_error("msm: null pointer"); return ZKHIP_EINVAL; }
  lane_hold H;
  if (H.rc != ZKHIP_OK) return H.rc;
  std::shared_ptr<registered_t> reg;
  size_t off = 0;
  if (n) { guard_t g(g_mu); reg = find_registered(bases, n, &off); }
  return host_msm(H, scalars, bases, n, reg, off, out_xyz);
}

// `batch` scalar vectors (contiguous, n elements each) against the same bases; out: batch Jacobian points.
// Registered bases in one shard: one batched launch set (window <= 16 bits) or pairs of overlapping MSMs (wide windows); otherwise one
// MSM per vector.
int zkhip_msm_g1_batch(const uint64_t* scalars, const uint64_t* bases, size_t n, size_t batch, uint64_t* out_xyz) {
  ZK_API_RANGE();
  if (!out_xyz || (n && batch && (!scalars || !bases))) { set_error("msm_batch: null pointer"); return ZKHIP_EINVAL; }
  if (batch == 0) return ZKHIP_OK;
  lane_hold H;
  if (H.rc != ZKHIP_OK) return H.rc;
  int rc;
  std::shared_ptr<registered_t> reg;
  size_t off = 0;
  if (n) { guard_t g(g_mu); reg = find_registered(bases, n, &off); }
  const shard_t* one = nullptr;
  if (reg) for (auto& sh : reg->shards) if (sh.dev == 0 && off >= sh.lo && off + n <= sh.lo + sh.n) one = &sh;
  if (!one || batch * 96 > LANE_PINNED || (one->pb->c > 16 && n * batch * 32 > ((size_t)4 << 30))) {   // (wide windows: the device path overlaps pairs of MSMs)
    for (size_t k = 0; k < batch; k++)
      if ((rc = host_msm(H, scalars + k * n * 4, bases, n, reg, off, out_xyz + k * 12)) != ZKHIP_OK) return rc;
    return ZKHIP_OK;
  }
  hipStream_t s = H.s;
  scratch* sc = H.sc;
  if ((rc = sc->scalars.reserve(n * batch * 32)) != ZKHIP_OK) return rc;
  if ((rc = sc->small.reserve(4096 + batch * 96)) != ZKHIP_OK) return rc;
  HIPCHK(hipMemcpyAsync(sc->scalars.p, scalars, n * batch * 32, hipMemcpyHostToDevice, s));
  {
    // reuse the handle-based entry point through a temporary handle for the registered table
    guard_t g(g_mu);
    const uint64_t tmp_handle = g_ctx.next_handle++;
    g_ctx.handles[tmp_handle] = one->pb;
    rc = zkhip_msm_g1_prepared_batch_device(tmp_handle, off - one->lo, sc->scalars.p, n, batch, n, sc->small.p, s);
    g_ctx.handles.erase(tmp_handle);
  }
  if (rc != ZKHIP_OK) return rc;
  HIPCHK(hipMemcpyAsync(H.L->pinned, sc->small.p, batch * 96, hipMemcpyDeviceToHost, s));
  if ((rc = H.finish()) != ZKHIP_OK) return rc;
  memcpy(out_xyz, H.L->pinned, batch * 96);
  return ZKHIP_OK;
}

int zkhip_register_bases(const uint64_t* bases, size_t n) {
  ZK_API_RANGE();
  if (!bases || n == 0) { set_error("register_bases: empty"); return ZKHIP_EINVAL; }
  {
    guard_t g(g_mu);
    int rc = ensure_init();
    if (rc != ZKHIP_OK) return rc;
    if (g_ctx.registered.count(bases)) zkhip_unregister_bases(bases);
  }
  lane_hold H;                                        // the primary device's uploads run on a borrowed lane
  if (H.rc != ZKHIP_OK) return H.rc;
  int S, ndev;
  { guard_t g(g_mu); S = g_ctx.shards; ndev = (int)g_ctx.devs.size(); }
  if ((size_t)S > n) S = (int)n;
  // shards on the other devices are uploaded through those devices' single lane, which a multi-device MSM of another thread drives
  // through its workers: the two take turns
  std::unique_lock<std::mutex> fan(g_fanout_mu, std::defer_lock);
  if (ndev > 1 && S > 1) fan.lock();
  auto reg = std::make_shared<registered_t>();
  reg->host = bases;
  reg->n = n;
  for (int i = 0; i < FINGER_POINTS; i++) {
    reg->finger_idx[i] = (size_t)((unsigned __int128)(n - 1) * (unsigned)i / (FINGER_POINTS - 1));
    memcpy(reg->finger[i], bases + reg->finger_idx[i] * 8, 64);
  }
  int rc = ZKHIP_OK;
  for (int s = 0; s < S && rc == ZKHIP_OK; s++) {
    size_t lo, hi;
    shard_range(n, s, S, &lo, &hi);
    if (lo >= hi) continue;
    const int di = s % ndev;
    device_ctx* D = g_ctx.devs[(size_t)di];
    std::unique_ptr<lane_hold> far(di == 0 ? nullptr : new lane_hold(*D));   // a secondary's lane for this shard (drained while its device is current)
    lane_hold& U = di == 0 ? H : *far;
    U.reopen();
    if (hipSetDevice(D->device) != hipSuccess) { set_error("hipSetDevice(%d) failed", D->device); rc = ZKHIP_ENODEV; break; }
    shard_t sh;
    sh.dev = di; sh.lo = lo; sh.n = hi - lo;
    if ((rc = U.sc->bases.reserve(sh.n * 64)) == ZKHIP_OK) {
      if (hipMemcpyAsync(U.sc->bases.p, bases + lo * 8, sh.n * 64, hipMemcpyHostToDevice, U.s) != hipSuccess) { set_error("register_bases: upload failed"); rc = ZKHIP_EHIP; }
      else rc = prepare_bases_device((const uint32_t*)U.sc->bases.p, sh.n, U.s, &sh.pb, 0, /* direct table only for arrays that are small as a whole: */ n);
    }
    if (rc == ZKHIP_OK) { reg->shards.push_back(sh); rc = U.finish(); }   // (the stream is idle: prepare_bases_device has waited for it)
  }
  (void)hipSetDevice(primary().device);
  if (rc != ZKHIP_OK) return rc;                      // ~registered_t frees the shards built so far
  guard_t g(g_mu);
  g_ctx.registered[bases] = reg;
  return ZKHIP_OK;
}

int zkhip_unregister_bases(const uint64_t* bases) {
  ZK_API_RANGE();
  std::shared_ptr<registered_t> reg;
  {
    guard_t g(g_mu);
    auto it = g_ctx.registered.find(bases);
    if (it == g_ctx.registered.end()) { set_error("unregister_bases: pointer not registered"); return ZKHIP_EINVAL; }
    reg = it->second;
    g_ctx.registered.erase(it);
    for (auto d : g_ctx.devs) { (void)hipSetDevice(d->device); (void)hipDeviceSynchronize(); }   // the tables may still be in use on a stream
    (void)hipSetDevice(primary().device);
  }
  return ZKHIP_OK;                                    // a host call still running holds its own reference; the last one frees the tables
}

int zkhip_prepare_bases_device(const void* d_bases, size_t n, uint64_t* handle) {
  ZK_API_RANGE();
  return zkhip_prepare_bases_device_c(d_bases, n, 0, handle);
}

int zkhip_prepare_bases_device_c(const void* d_bases, size_t n, int window_bits, uint64_t* handle) {
  ZK_API_RANGE();
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  if (!d_bases || !handle || n == 0) { set_error("prepare_bases: bad argument"); return ZKHIP_EINVAL; }
  prepared_bases* pb = nullptr;
  HIPCHK(hipDeviceSynchronize());           // d_bases may still be being written on the caller's stream; one-time call
  if ((rc = prepare_bases_device((const uint32_t*)d_bases, n, nullptr, &pb, window_bits)) != ZKHIP_OK) return rc;
  *handle = g_ctx.next_handle++;
  g_ctx.handles[*handle] = pb;
  return ZKHIP_OK;
}

int zkhip_release_bases(uint64_t handle) {
  guard_t g(g_mu);
  auto it = g_ctx.handles.find(handle);
  if (it == g_ctx.handles.end()) { set_error("release_bases: unknown handle"); return ZKHIP_EINVAL; }
  (void)hipDeviceSynchronize();
  release_prepared(it->second);
  g_ctx.handles.erase(it);
  return ZKHIP_OK;
}

int zkhip_prepared_window_bits(uint64_t handle) {
  guard_t g(g_mu);
  auto it = g_ctx.handles.find(handle);
  if (it == g_ctx.handles.end()) { set_error("prepared_window_bits: unknown handle"); return ZKHIP_EINVAL; }
  return it->second->c;
}

int zkhip_msm_g1_prepared_device(uint64_t handle, size_t offset, const void* d_scalars, size_t n, void* d_out_xyz, void* stream) {
  ZK_API_RANGE();
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  auto it = g_ctx.handles.find(handle);
  if (it == g_ctx.handles.end()) { set_error("msm_prepared: unknown handle"); return ZKHIP_EINVAL; }
  if (!d_out_xyz || (n && !d_scalars)) { set_error("msm_prepared: null pointer"); return ZKHIP_EINVAL; }
  const prepared_bases* pb = it->second;
  hipStream_t s = caller_stream(stream);
  scratch* sc = scratch_for(primary(), s);
  if ((rc = sc->ws.reserve(msm_workspace_bytes(n, pb->c, true))) != ZKHIP_OK) return rc;
  return msm_g1_device((const uint32_t*)d_scalars, nullptr, n, (uint32_t*)d_out_xyz, sc->ws.p, sc->ws.cap, 0, s, pb, offset);
}

}  // extern "C"

namespace zkhip {

// `batch` prepared MSMs of n points each on one device (current device = pb's), results at d_out + k * 24 words: tables with windows of
// <= 16 bits share launch sets (groups of vectors, each with its own bucket set), wider ones run one vector after the other.
// vectors of a batch that share one launch set: all of them for windows <= 16 bits, within 2^31 sorted entries and 4 Mi buckets
static size_t batch_group(const prepared_bases* pb, size_t n, size_t batch) {
  size_t group = (pb->c > 16 || batch <= 1) ? 1 : std::min<size_t>(batch, 65535);
  while (group > 1 && ((size_t)((256 + pb->c - 1) / pb->c) * n * group >= (1ull << 31) || (group << (pb->c - 1)) > (1ull << 22))) group = (group + 1) / 2;
  return group;
}

static int prepared_batch_enqueue(scratch* sc, hipStream_t s, const prepared_bases* pb, size_t pb_off, const uint32_t* d_scalars, size_t n, size_t batch,
                                  size_t scalar_stride, uint32_t* d_out) {
  int rc;
  const size_t group = batch_group(pb, n, batch);
  if ((rc = sc->ws.reserve(msm_workspace_bytes(n, pb->c, true, group))) != ZKHIP_OK) return rc;
  for (size_t k0 = 0; k0 < batch; k0 += group) {
    const size_t kk = batch - k0 < group ? batch - k0 : group;
    rc = msm_g1_device(d_scalars + k0 * scalar_stride * 8, nullptr, n, d_out + k0 * 24, sc->ws.p, sc->ws.cap, 0, s, pb, pb_off, kk, scalar_stride);
    if (rc != ZKHIP_OK) return rc;
  }
  return ZKHIP_OK;
}

// Device-resident scalars (primary device, caller's stream s) against a registered array whose range [off, off + n) spans several shards
// (SURVEY.md section 8(e) partitioning, with the scalars already in HBM): every shard the range touches runs its own prepared Pippenger on
// its device.  The primary device's pieces run on s.  A secondary device waits for the scalars (event on s), pulls its slice of every
// vector from the primary's HBM over xGMI (hipMemcpyPeerAsync: 32 B x n / S per vector -- 64 MiB per GPU for configs[4], about a
// millisecond beside a 2.9 ms shard MSM), runs its pieces on its own stream and sends each 96-byte partial back into the gather buffer of
// the caller's stream; s waits for the secondaries' events (fan_call) and folds: out[k] = sum over pieces of partial[piece][k].  Asynchronous like
// every `_device` call: nothing here waits for a device unless the call fails half-way.  g_mu held by the caller.
static int registered_device_msm(const std::shared_ptr<registered_t>& reg, size_t off, const uint32_t* d_scalars, size_t n, size_t batch, size_t stride,
                                 uint32_t* d_out, hipStream_t s) {
  int rc;
  device_ctx& P = primary();
  scratch* sc = scratch_for(P, s);
  std::vector<piece_t> pieces;
  for (auto& sh : reg->shards) {
    const size_t lo = std::max(off, sh.lo), hi = std::min(off + n, sh.lo + sh.n);
    if (lo < hi) pieces.push_back({sh.dev, lo - off, hi - lo, sh.pb, lo - sh.lo});
  }
  if (pieces.size() == 1 && pieces[0].dev == 0)
    return prepared_batch_enqueue(sc, s, pieces[0].pb, pieces[0].pb_off, d_scalars, n, batch, stride, d_out);
  const size_t np = pieces.size();
  if ((rc = sc->gather.reserve(np * batch * 96)) != ZKHIP_OK) return rc;
  uint32_t* gather = (uint32_t*)sc->gather.p;                     // [piece][vector] 96-byte slots
  fan_call F;
  if ((rc = F.begin(s)) != ZKHIP_OK) return rc;
  // the secondaries first: their copies and kernels start while this thread is still enqueueing the primary's pieces
  for (size_t d = 1; d < g_ctx.devs.size(); d++) {
    std::vector<size_t> mine;
    for (size_t i = 0; i < np; i++) if ((size_t)pieces[i].dev == d) mine.push_back(i);
    if (mine.empty()) continue;
    device_ctx* D = g_ctx.devs[d];
    if ((rc = F.dev((int)d)) != ZKHIP_OK) return rc;
    hipStream_t fs = F.st[d];
    scratch* dsc = scratch_for(*D, fs);
    size_t sc_elems = 0;
    for (size_t i : mine) sc_elems = std::max(sc_elems, pieces[i].n);
    if ((rc = dsc->scalars.reserve(sc_elems * batch * 32)) != ZKHIP_OK) return rc;
    if ((rc = dsc->small.reserve(4096 + batch * 96)) != ZKHIP_OK) return rc;
    size_t ws_bytes = 0;                                          // sized once for the largest piece (growing it later would free it under queued work)
    for (size_t i : mine) ws_bytes = std::max(ws_bytes, msm_workspace_bytes(pieces[i].n, pieces[i].pb->c, true, batch_group(pieces[i].pb, pieces[i].n, batch)));
    if ((rc = dsc->ws.reserve(ws_bytes)) != ZKHIP_OK) return rc;
    for (size_t i : mine) {
      const piece_t& p = pieces[i];
      uint32_t* slice = (uint32_t*)dsc->scalars.p;                // vector k of this piece at slice + k * p.n * 8 words
      for (size_t k = 0; k < batch; k++)
        HIPCHK(hipMemcpyPeerAsync(slice + k * p.n * 8, D->device, d_scalars + (k * stride + p.lo) * 8, P.device, p.n * 32, fs));
      uint32_t* part = (uint32_t*)((char*)dsc->small.p + 4096);
      if ((rc = prepared_batch_enqueue(dsc, fs, p.pb, p.pb_off, slice, p.n, batch, p.n, part)) != ZKHIP_OK) return rc;
      HIPCHK(hipMemcpyPeerAsync(gather + i * batch * 24, P.device, part, D->device, batch * 96, fs));
    }
  }
  if ((rc = F.dev(0)) != ZKHIP_OK) return rc;
  size_t ws_bytes = 0;
  for (auto& p : pieces) if (p.dev == 0) ws_bytes = std::max(ws_bytes, msm_workspace_bytes(p.n, p.pb->c, true, batch_group(p.pb, p.n, batch)));
  if ((rc = sc->ws.reserve(ws_bytes)) != ZKHIP_OK) return rc;
  for (size_t i = 0; i < np; i++) {
    const piece_t& p = pieces[i];
    if (p.dev == 0 && (rc = prepared_batch_enqueue(sc, s, p.pb, p.pb_off, d_scalars + p.lo * 8, p.n, batch, stride, gather + i * batch * 24)) != ZKHIP_OK) return rc;
  }
  if ((rc = F.end()) != ZKHIP_OK) return rc;
  return sum_jacobian_device(gather, (int)np, d_out, s, batch);
}

}  // namespace zkhip

extern "C" {

// device-resident scalars against bases pinned with zkhip_register_bases (`bases` = a host pointer into a registered array): the commit
// of a polynomial that lives in HBM against the SRS the host registered, without a second table (zkhip_prepare_bases_device).  A range
// that spans several shards fans out over their devices (registered_device_msm above).
int zkhip_msm_g1_registered_batch_device(const uint64_t* bases, const void* d_scalars, size_t n, size_t batch, size_t scalar_stride, void* d_out_xyz,
                                         void* stream) {
  ZK_API_RANGE();
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  if (batch == 0) return ZKHIP_OK;
  if (!d_out_xyz || (n && (!d_scalars || !bases)) || (batch > 1 && scalar_stride < n)) { set_error("msm_registered: bad argument"); return ZKHIP_EINVAL; }
  hipStream_t s = caller_stream(stream);
  if (n == 0) return msm_g1_device(nullptr, nullptr, 0, (uint32_t*)d_out_xyz, nullptr, 0, 0, s, nullptr, 0, batch, 0);
  size_t off = 0;
  std::shared_ptr<registered_t> reg = find_registered(bases, n, &off);
  if (!reg) { set_error("msm_registered: the range is not inside a registered array"); return ZKHIP_EINVAL; }
  // the tables outlive the enqueued work: zkhip_unregister_bases synchronises every device before the last reference goes
  return registered_device_msm(reg, off, (const uint32_t*)d_scalars, n, batch, scalar_stride, (uint32_t*)d_out_xyz, s);
}

int zkhip_msm_g1_registered_device(const uint64_t* bases, const void* d_scalars, size_t n, void* d_out_xyz, void* stream) {
  ZK_API_RANGE();
  return zkhip_msm_g1_registered_batch_device(bases, d_scalars, n, 1, n, d_out_xyz, stream);
}

int zkhip_msm_g1_prepared_batch_device(uint64_t handle, size_t offset, const void* d_scalars, size_t n, size_t batch, size_t scalar_stride,
                                       void* d_out_xyz, void* stream) {
  ZK_API_RANGE();
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  auto it = g_ctx.handles.find(handle);
  if (it == g_ctx.handles.end()) { set_error("msm_prepared_batch: unknown handle"); return ZKHIP_EINVAL; }
  if (!d_out_xyz || (n && batch && !d_scalars) || (batch > 1 && scalar_stride < n)) { set_error("msm_prepared_batch: bad argument"); return ZKHIP_EINVAL; }
  const prepared_bases* pb = it->second;
  hipStream_t s = caller_stream(stream);
  scratch* sc = scratch_for(primary(), s);
  // tables built for wide windows (n >= 2^20) do not batch: those MSMs are throughput-bound one at a time
  size_t group = (pb->c > 16 || batch <= 1) ? 1 : batch;
  while (group > 1 && ((size_t)((256 + pb->c - 1) / pb->c) * n * group >= (1ull << 31) || (group << (pb->c - 1)) > (1ull << 22))) group = (group + 1) / 2;   // <= 4 Mi buckets per launch set
  if (group == 1 && batch > 1 && n >= ((size_t)1 << 18)) {
    // Large MSMs do not share a launch set, but two of them overlap: while one is in its latency-bound sort and reduction tail the
    // other's accumulation fills the chip (measured: 2^20 1.50 -> 1.30 ms, 2^22 5.26 -> 4.87 ms per MSM).  Odd vectors go to a
    // library-owned high-priority stream (streams of different priority never share a hardware queue) forked from / joined to the
    // caller's stream with events; each stream has its own scratch set.
    device_ctx& P = primary();
    if (!P.side) {
      int lo = 0, hi = 0;
      (void)hipDeviceGetStreamPriorityRange(&lo, &hi);          // hi = numerically lowest = greatest priority
      HIPCHK(hipStreamCreateWithPriority(&P.side, hipStreamNonBlocking, hi));
      HIPCHK(hipEventCreateWithFlags(&P.side_fork, hipEventDisableTiming));
      HIPCHK(hipEventCreateWithFlags(&P.side_join, hipEventDisableTiming));
    }
    scratch* sc2 = scratch_for(P, P.side);
    const size_t ws_bytes = msm_workspace_bytes(n, pb->c, true, 1);
    if ((rc = sc->ws.reserve(ws_bytes)) != ZKHIP_OK) return rc;
    if ((rc = sc2->ws.reserve(ws_bytes)) != ZKHIP_OK) return rc;
    HIPCHK(hipEventRecord(P.side_fork, s));
    HIPCHK(hipStreamWaitEvent(P.side, P.side_fork, 0));
    for (size_t k0 = 0; k0 < batch; k0++) {
      const bool on_side = (k0 & 1) != 0;
      scratch* use = on_side ? sc2 : sc;
      rc = msm_g1_device((const uint32_t*)d_scalars + k0 * scalar_stride * 8, nullptr, n, (uint32_t*)d_out_xyz + k0 * 24, use->ws.p, use->ws.cap, 0, on_side ? P.side : s, pb,
                         offset, 1, scalar_stride);
      if (rc != ZKHIP_OK) break;
    }
    HIPCHK(hipEventRecord(P.side_join, P.side));               // also on an error: the caller's stream must not run ahead of the side stream
    HIPCHK(hipStreamWaitEvent(s, P.side_join, 0));
    return rc;
  }
  for (size_t k0 = 0; k0 < batch; k0 += group) {
    const size_t kk = batch - k0 < group ? batch - k0 : group;
    if ((rc = sc->ws.reserve(msm_workspace_bytes(n, pb->c, true, kk))) != ZKHIP_OK) return rc;
    rc = msm_g1_device((const uint32_t*)d_scalars + k0 * scalar_stride * 8, nullptr, n, (uint32_t*)d_out_xyz + k0 * 24, sc->ws.p, sc->ws.cap, 0, s, pb,
                       offset, kk, scalar_stride);
    if (rc != ZKHIP_OK) return rc;
  }
  return ZKHIP_OK;
}

int zkhip_g1_sum_device(const void* d_points_xyz, int m, void* d_out_xyz, void* stream) {
  ZK_API_RANGE();
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  if (m < 0 || !d_out_xyz || (m && !d_points_xyz)) { set_error("g1_sum: bad argument"); return ZKHIP_EINVAL; }
  return sum_jacobian_device((const uint32_t*)d_points_xyz, m, (uint32_t*)d_out_xyz, caller_stream(stream));
}

int zkhip_g1_sum(const uint64_t* points_xyz, int m, uint64_t out_xyz[12]) {
  ZK_API_RANGE();
  if (m < 0 || !out_xyz || (m && !points_xyz)) { set_error("g1_sum: bad argument"); return ZKHIP_EINVAL; }
  lane_hold H;
  if (H.rc != ZKHIP_OK) return H.rc;
  int rc;
  if ((rc = H.sc->small.reserve(4096 + (size_t)m * 96)) != ZKHIP_OK) return rc;
  char* d = (char*)H.sc->small.p;
  if (m) HIPCHK(hipMemcpyAsync(d + 4096, points_xyz, (size_t)m * 96, hipMemcpyHostToDevice, H.s));
  if ((rc = sum_jacobian_device((const uint32_t*)(d + 4096), m, (uint32_t*)d, H.s)) != ZKHIP_OK) return rc;
  HIPCHK(hipMemcpyAsync(H.L->pinned, d, 96, hipMemcpyDeviceToHost, H.s));
  if ((rc = H.finish()) != ZKHIP_OK) return rc;
  memcpy(out_xyz, H.L->pinned, 96);
  return ZKHIP_OK;
}

}  // extern "C"

namespace zkhip {

// ---- NTT / domain ----------------------------------------------------------------------------------
// runs ntt_transform with scratch from the stream's set (two buffers of batch * 2^L elements when the transform is multi-pass)
static int run_transform(scratch* sc, const uint32_t* d_in, uint32_t in_len, uint32_t in_stride, uint32_t* d_out, uint32_t out_len, uint32_t out_stride,
                         uint32_t batch, uint32_t L, const uint32_t* omega, const uint32_t* in_scale, uint32_t in_period,
                         const uint32_t* out_scale, uint32_t out_period, hipStream_t s) {
  if (L > 28) { set_error("ntt: log_n = %u > 28", L); return ZKHIP_EINVAL; }
  const int np = ntt_passes(L);
  // the passes ping-pong through one or two scratch copies of the batch: cap the scratch at ~2 GiB per copy by transforming a large
  // batch in sub-batches (same kernels, same throughput; 26 polynomials of 2^24 would otherwise need 28 GB of scratch)
  uint32_t sub = batch;
  const size_t cap = (size_t)1 << 31;
  if (batch > 1 && (((size_t)batch << L) * 32) > cap) sub = (uint32_t)std::max<size_t>(1, cap / (((size_t)1 << L) * 32));
  const size_t one = (size_t)sub << L;     // elements per scratch copy
  uint32_t *t0 = nullptr, *t1 = nullptr;
  if (np >= 2) {
    int rc = sc->ntt_tmp.reserve(one * 32 * (np >= 3 ? 2 : 1));
    if (rc != ZKHIP_OK) return rc;
    t0 = (uint32_t*)sc->ntt_tmp.p;
    if (np >= 3) t1 = t0 + one * 8;
  }
  for (uint32_t b0 = 0; b0 < batch; b0 += sub) {
    const uint32_t nb = batch - b0 < sub ? batch - b0 : sub;
    int rc = ntt_transform(d_in + (size_t)b0 * in_stride * 8, in_len, in_stride, d_out + (size_t)b0 * out_stride * 8, out_len, out_stride, nb, L, omega,
                           in_scale, in_period, out_scale, out_period, t0, t1, s);
    if (rc != ZKHIP_OK) return rc;
  }
  return ZKHIP_OK;
}

// a `_device` transform on the caller's stream (g_mu held by the caller)
static int device_transform_one(const void* d_in, uint32_t in_len, size_t in_stride, void* d_out, uint32_t out_len, size_t out_stride, uint32_t batch, uint32_t L,
                                const uint64_t* omega, const uint32_t* in_scale, uint32_t in_period, const uint32_t* out_scale, uint32_t out_period, hipStream_t s) {
  return run_transform(scratch_for(primary(), s), (const uint32_t*)d_in, in_len, (uint32_t)in_stride, (uint32_t*)d_out, out_len, (uint32_t)out_stride, batch, L,
                       (const uint32_t*)omega, in_scale, in_period, out_scale, out_period, s);
}

// Round 5 (second split): the polynomials of a batch are independent units, so a batched transform may be spread over the
// devices of zkhip_init -- every transform still runs on ONE device.  Polynomials [lo_d, hi_d) (shard_range over the batch) go to device d.
// `_device` form (this function, fan-out mode 2 only; the protocol is fan_call's): device d > 0 waits for the caller's stream, pulls its polynomials
// from the primary's HBM over xGMI (hipMemcpyPeerAsync) into its own scratch, transforms them on its own stream with its own twiddle plan and pushes
// the results back into d_out; the caller's stream waits for it.  Asynchronous like every `_device` call.
// Off by default: a 2^24 result is 512 MiB over one xGMI link (about 8 ms at 65 GB/s) against a 1.8 ms transform, so copying out and back
// only pays where the links are idle and the batch is deep; the host-buffer forms below (mode 1, default) are the ones that win outright --
// each device moves its own polynomials over its own PCIe link.  Results are identical either way (one device per transform).
static int device_transform(const void* d_in, uint32_t in_len, size_t in_stride, void* d_out, uint32_t out_len, size_t out_stride, uint32_t batch, uint32_t L,
                            const uint64_t* omega, const uint32_t* in_scale, uint32_t in_period, const uint32_t* out_scale, uint32_t out_period, void* stream) {
  hipStream_t s = caller_stream(stream);
  const int S = (int)g_ctx.devs.size();
  if (g_ctx.ntt_fanout < 2 || S < 2 || batch < 2 || L < 12)
    return device_transform_one(d_in, in_len, in_stride, d_out, out_len, out_stride, batch, L, omega, in_scale, in_period, out_scale, out_period, s);
  device_ctx& P = primary();
  const size_t N = (size_t)1 << L;
  int rc;
  fan_call F;
  if ((rc = F.begin(s)) != ZKHIP_OK) return rc;
  for (int d = 1; d < S; d++) {
    size_t lo, hi;
    shard_range(batch, d, S, &lo, &hi);
    if (lo >= hi) continue;
    device_ctx* D = g_ctx.devs[(size_t)d];
    if ((rc = F.dev(d)) != ZKHIP_OK) return rc;
    hipStream_t fs = F.st[(size_t)d];
    scratch* dsc = scratch_for(*D, fs);
    const size_t cnt = hi - lo;
    if ((rc = dsc->poly.reserve(cnt * N * 32)) != ZKHIP_OK) return rc;
    uint32_t* buf = (uint32_t*)dsc->poly.p;                   // polynomial b of this device at buf + b * N elements, transformed in place
    for (size_t b = 0; b < cnt; b++)
      HIPCHK(hipMemcpyPeerAsync(buf + b * N * 8, D->device, (const uint32_t*)d_in + (lo + b) * in_stride * 8, P.device, (size_t)in_len * 32, fs));
    if ((rc = run_transform(dsc, buf, in_len, (uint32_t)N, buf, out_len, (uint32_t)N, (uint32_t)cnt, L, (const uint32_t*)omega, in_scale, in_period, out_scale,
                            out_period, fs)) != ZKHIP_OK) return rc;
    for (size_t b = 0; b < cnt; b++)
      HIPCHK(hipMemcpyPeerAsync((uint32_t*)d_out + (lo + b) * out_stride * 8, P.device, buf + b * N * 8, D->device, (size_t)out_len * 32, fs));
  }
  if ((rc = F.dev(0)) != ZKHIP_OK) return rc;
  size_t lo, hi;
  shard_range(batch, 0, S, &lo, &hi);
  if (lo < hi && (rc = device_transform_one((const uint32_t*)d_in + lo * in_stride * 8, in_len, in_stride, (uint32_t*)d_out + lo * out_stride * 8, out_len, out_stride,
                                            (uint32_t)(hi - lo), L, omega, in_scale, in_period, out_scale, out_period, s)) != ZKHIP_OK) return rc;
  return F.end();
}

}  // namespace zkhip

extern "C" {

int zkhip_ntt_fr_batch_device(void* d_a, const uint64_t omega[4], uint32_t log_n, uint32_t batch, size_t stride, void* stream) {
  ZK_API_RANGE();
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  if (!d_a || !omega || log_n > 28 || stride < ((size_t)1 << log_n) || stride >= ((size_t)1 << 32)) { set_error("ntt_batch: bad argument"); return ZKHIP_EINVAL; }
  const uint32_t N = 1u << log_n;
  return device_transform(d_a, N, stride, d_a, N, stride, batch, log_n, omega, nullptr, 0, nullptr, 0, stream);
}

int zkhip_ifft_scaled_batch_device(void* d_a, const uint64_t omega_inv[4], uint32_t log_n, const uint64_t divisor[4], uint32_t batch, size_t stride,
                                   void* stream) {
  ZK_API_RANGE();
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  if (!d_a || !omega_inv || !divisor || log_n > 28 || stride < ((size_t)1 << log_n) || stride >= ((size_t)1 << 32)) { set_error("ifft_batch: bad argument"); return ZKHIP_EINVAL; }
  const uint32_t N = 1u << log_n;
  return device_transform(d_a, N, stride, d_a, N, stride, batch, log_n, omega_inv, nullptr, 0, (const uint32_t*)divisor, 1, stream);
}

int zkhip_ntt_fr_device(void* d_a, const uint64_t omega[4], uint32_t log_n, void* stream) {
  ZK_API_RANGE();
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  if (!d_a || !omega) { set_error("ntt: null pointer"); return ZKHIP_EINVAL; }
  if (log_n > 28) { set_error("ntt: log_n = %u > 28", log_n); return ZKHIP_EINVAL; }
  const uint32_t N = 1u << log_n;
  return device_transform(d_a, N, N, d_a, N, N, 1, log_n, omega, nullptr, 0, nullptr, 0, stream);
}

int zkhip_ifft_scaled_device(void* d_a, const uint64_t omega_inv[4], uint32_t log_n, const uint64_t divisor[4], void* stream) {
  ZK_API_RANGE();
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  if (!d_a || !omega_inv || !divisor) { set_error("ifft: null pointer"); return ZKHIP_EINVAL; }
  if (log_n > 28) { set_error("ifft: log_n = %u > 28", log_n); return ZKHIP_EINVAL; }
  const uint32_t N = 1u << log_n;
  return device_transform(d_a, N, N, d_a, N, N, 1, log_n, omega_inv, nullptr, 0, (const uint32_t*)divisor, 1, stream);
}

int zkhip_mul_periodic_device(void* d_a, size_t n, const void* d_table, uint32_t period, void* stream) {
  ZK_API_RANGE();
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  if ((n && !d_a) || !d_table) { set_error("mul_periodic: null pointer"); return ZKHIP_EINVAL; }
  return fr_mul_periodic_device((uint32_t*)d_a, n, (const uint32_t*)d_table, period, caller_stream(stream));
}

}  // extern "C"

namespace zkhip {

// One device's share of a host-buffer batch on the held lane H: `cnt` polynomials (polynomial b at in + b * in_stride elements) cross this
// device's PCIe link into its scratch, are transformed in place (polynomial b at b * N elements) and go back to out + b * out_stride.  Runs on the
// calling thread for the primary device and on the device's worker thread for a secondary (the current device is per host thread).
static int host_transform_share(lane_hold& H, const uint64_t* in, size_t in_len, size_t in_stride, uint64_t* out, size_t out_len, size_t out_stride,
                                size_t cnt, uint32_t log_n, const uint64_t* omega, const uint32_t* in_scale, uint32_t in_period, const uint32_t* out_scale,
                                uint32_t out_period) {
  int rc;
  scratch* const sc = H.sc;
  hipStream_t s = H.s;
  const size_t N = (size_t)1 << log_n;
  if ((rc = sc->poly.reserve(cnt * N * 32)) != ZKHIP_OK) return rc;
  if (cnt == 1) HIPCHK(hipMemcpyAsync(sc->poly.p, in, in_len * 32, hipMemcpyHostToDevice, s));
  else if (in_len == N && in_stride == N) HIPCHK(hipMemcpyAsync(sc->poly.p, in, cnt * N * 32, hipMemcpyHostToDevice, s));
  else HIPCHK(hipMemcpy2DAsync(sc->poly.p, N * 32, in, in_stride * 32, in_len * 32, cnt, hipMemcpyHostToDevice, s));
  rc = run_transform(sc, (const uint32_t*)sc->poly.p, (uint32_t)in_len, (uint32_t)N, (uint32_t*)sc->poly.p, (uint32_t)out_len, (uint32_t)N, (uint32_t)cnt, log_n,
                     (const uint32_t*)omega, in_scale, in_period, out_scale, out_period, s);
  if (rc != ZKHIP_OK) return rc;
  if (cnt == 1) HIPCHK(hipMemcpyAsync(out, sc->poly.p, out_len * 32, hipMemcpyDeviceToHost, s));
  else if (out_len == N && out_stride == N) HIPCHK(hipMemcpyAsync(out, sc->poly.p, cnt * N * 32, hipMemcpyDeviceToHost, s));
  else HIPCHK(hipMemcpy2DAsync(out, out_stride * 32, sc->poly.p, N * 32, out_len * 32, cnt, hipMemcpyDeviceToHost, s));
  return H.finish();
}

// Host-buffer transforms, `batch` polynomials.  With several devices (fan-out mode >= 1) the batch is cut by shard_range: the primary's share
// runs on this thread's lane, every other device's share on its worker thread -- N PCIe links carry the batch instead of one (a 2^24
// transform through ONE link is 21 ms around a 1.8 ms kernel).  Each transform runs on one device: the results do not depend on the split.
static int host_transform(const uint64_t* in, size_t in_len, size_t in_stride, uint64_t* out, size_t out_len, size_t out_stride, uint32_t batch, uint32_t log_n,
                          const uint64_t* omega, const uint32_t* in_scale, uint32_t in_period, const uint32_t* out_scale, uint32_t out_period) {
  if (log_n > 28) { set_error("ntt: log_n = %u > 28", log_n); return ZKHIP_EINVAL; }
  if (!in || !out || !omega) { set_error("ntt: null pointer"); return ZKHIP_EINVAL; }
  const size_t N = (size_t)1 << log_n;
  if (in_len > N || out_len > N || (batch > 1 && (in_stride < in_len || out_stride < out_len))) { set_error("ntt: length exceeds domain or stride"); return ZKHIP_EINVAL; }
  if (batch == 0) return ZKHIP_OK;
  lane_hold H;
  if (H.rc != ZKHIP_OK) return H.rc;
  int S, mode;
  { guard_t g(g_mu); S = (int)g_ctx.devs.size(); mode = g_ctx.ntt_fanout; }
  if (S < 2 || batch < 2 || mode < 1)
    return host_transform_share(H, in, in_len, in_stride, out, out_len, out_stride, batch, log_n, omega, in_scale, in_period, out_scale, out_period);
  std::unique_lock<std::mutex> fan(g_fanout_mu);              // the secondary devices have one lane each
  for (int d = 1; d < S; d++) {
    size_t lo, hi;
    shard_range(batch, d, S, &lo, &hi);
    if (lo >= hi) continue;
    device_ctx* D = g_ctx.devs[(size_t)d];
    D->w->submit([=]() -> int {
      lane_hold U(*D);                                     // a failed job has drained the lane before wait() hands its error to the caller
      return host_transform_share(U, in + lo * in_stride * 4, in_len, in_stride, out + lo * out_stride * 4, out_len, out_stride, hi - lo, log_n, omega,
                                  in_scale, in_period, out_scale, out_period);
    });
  }
  int rc_local = ZKHIP_OK;
  {
    size_t lo, hi;
    shard_range(batch, 0, S, &lo, &hi);
    if (lo < hi)
      rc_local = host_transform_share(H, in + lo * in_stride * 4, in_len, in_stride, out + lo * out_stride * 4, out_len, out_stride, hi - lo, log_n, omega,
                                      in_scale, in_period, out_scale, out_period);
  }
  int rc_remote = ZKHIP_OK;
  for (int d = 1; d < S; d++) {
    size_t lo, hi;
    shard_range(batch, d, S, &lo, &hi);
    if (lo >= hi) continue;
    const int r = g_ctx.devs[(size_t)d]->w->wait();
    if (r != ZKHIP_OK) rc_remote = r;
  }
  return rc_local != ZKHIP_OK ? rc_local : rc_remote;
}

}  // namespace zkhip

extern "C" {

int zkhip_set_ntt_fanout(int mode) {
  ZK_API_RANGE();
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  if (mode < 0 || mode > 2) { set_error("set_ntt_fanout: mode %d not in 0..2", mode); return ZKHIP_EINVAL; }
  g_ctx.ntt_fanout = mode;
  return ZKHIP_OK;
}

int zkhip_ntt_fanout(void) {
  guard_t g(g_mu);
  return g_ctx.ready ? g_ctx.ntt_fanout : 1;
}

// `batch` contiguous polynomials of 2^log_n elements, transformed in place (one launch set per device)
int zkhip_ntt_fr_batch(uint64_t* a, const uint64_t omega[4], uint32_t log_n, uint32_t batch) {
  ZK_API_RANGE();
  if (!a || !omega || log_n > 28) { set_error("ntt_batch: bad argument"); return ZKHIP_EINVAL; }
  const size_t N = (size_t)1 << log_n;
  return host_transform(a, N, N, a, N, N, batch, log_n, omega, nullptr, 0, nullptr, 0);
}

int zkhip_ifft_scaled_batch(uint64_t* a, const uint64_t omega_inv[4], uint32_t log_n, const uint64_t divisor[4], uint32_t batch) {
  ZK_API_RANGE();
  if (!a || !omega_inv || !divisor || log_n > 28) { set_error("ifft_batch: bad argument"); return ZKHIP_EINVAL; }
  const size_t N = (size_t)1 << log_n;
  return host_transform(a, N, N, a, N, N, batch, log_n, omega_inv, nullptr, 0, (const uint32_t*)divisor, 1);
}

int zkhip_ntt_fr(uint64_t* a, const uint64_t omega[4], uint32_t log_n) {
  ZK_API_RANGE();
  const size_t N = (size_t)1 << (log_n > 28 ? 0 : log_n);
  return host_transform(a, N, N, a, N, N, 1, log_n, omega, nullptr, 0, nullptr, 0);
}

int zkhip_ifft_scaled(uint64_t* a, const uint64_t omega_inv[4], uint32_t log_n, const uint64_t divisor[4]) {
  ZK_API_RANGE();
  if (!divisor) { set_error("ifft: null divisor"); return ZKHIP_EINVAL; }
  const size_t N = (size_t)1 << (log_n > 28 ? 0 : log_n);
  return host_transform(a, N, N, a, N, N, 1, log_n, omega_inv, nullptr, 0, (const uint32_t*)divisor, 1);
}

}  // extern "C"

namespace zkhip {
// scale triples of the coset transforms, computed on the host (4 x 64 Montgomery, include/zkhip.hpp):
//   into the coset:   {1, zeta, zeta^2}                      (distribute_powers_zeta(.., true): [g_coset, g_coset_inv])
//   out of the coset: divisor * {1, zeta^2, zeta}            (distribute_powers_zeta(.., false) + the ifft divisor)
static void coset_scales(const uint64_t zeta[4], const uint64_t* divisor, uint32_t out[24]) {
  namespace hd = zkhip::halo2::detail;
  zkhip::halo2::Fr z, zz, c0;
  memcpy(z.l, zeta, 32);
  zz = hd::mul(z, z);
  if (!divisor) {
    c0 = hd::one();
    memcpy(out, c0.l, 32); memcpy(out + 8, z.l, 32); memcpy(out + 16, zz.l, 32);
  } else {
    memcpy(c0.l, divisor, 32);
    const zkhip::halo2::Fr c1 = hd::mul(c0, zz), c2 = hd::mul(c0, z);
    memcpy(out, c0.l, 32); memcpy(out + 8, c1.l, 32); memcpy(out + 16, c2.l, 32);
  }
}
}  // namespace zkhip

extern "C" {

int zkhip_coeff_to_extended(const uint64_t* a, uint32_t k, uint64_t* out, uint32_t ext_k, const uint64_t ext_omega[4], const uint64_t zeta[4]) {
  ZK_API_RANGE();
  if (!a || !out || !ext_omega || !zeta || k > ext_k || ext_k > 28) { set_error("coeff_to_extended: bad argument"); return ZKHIP_EINVAL; }
  uint32_t sc[24];
  coset_scales(zeta, nullptr, sc);
  return host_transform(a, (size_t)1 << k, (size_t)1 << k, out, (size_t)1 << ext_k, (size_t)1 << ext_k, 1, ext_k, ext_omega, sc, 3, nullptr, 0);
}

// `batch` polynomials: polynomial b = a[b * 2^k ..], its extended-coset evaluations = out[b * 2^ext_k ..] (the per-column loop of the
// quotient phase in one call; with several devices each takes its share of the columns over its own PCIe link)
int zkhip_coeff_to_extended_batch(const uint64_t* a, uint32_t k, uint64_t* out, uint32_t ext_k, uint32_t batch, const uint64_t ext_omega[4],
                                  const uint64_t zeta[4]) {
  ZK_API_RANGE();
  if (!a || !out || !ext_omega || !zeta || k > ext_k || ext_k > 28) { set_error("coeff_to_extended_batch: bad argument"); return ZKHIP_EINVAL; }
  uint32_t sc[24];
  coset_scales(zeta, nullptr, sc);
  return host_transform(a, (size_t)1 << k, (size_t)1 << k, out, (size_t)1 << ext_k, (size_t)1 << ext_k, batch, ext_k, ext_omega, sc, 3, nullptr, 0);
}

int zkhip_extended_to_coeff(uint64_t* a, uint32_t ext_k, const uint64_t ext_omega_inv[4], const uint64_t ext_divisor[4],
                            const uint64_t zeta[4], uint64_t* out, size_t out_len) {
  ZK_API_RANGE();
  if (!a || !out || !ext_omega_inv || !ext_divisor || !zeta || ext_k > 28) { set_error("extended_to_coeff: bad argument"); return ZKHIP_EINVAL; }
  uint32_t sc[24];
  coset_scales(zeta, ext_divisor, sc);
  return host_transform(a, (size_t)1 << ext_k, (size_t)1 << ext_k, out, out_len, out_len, 1, ext_k, ext_omega_inv, nullptr, 0, sc, 3);
}

// device-resident forms, `batch` polynomials per launch set (polynomial b at base + b * stride elements)
int zkhip_coeff_to_extended_device(const void* d_a, size_t a_stride, uint32_t k, void* d_out, size_t out_stride, uint32_t ext_k, uint32_t batch,
                                   const uint64_t ext_omega[4], const uint64_t zeta[4], void* stream) {
  ZK_API_RANGE();
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  if (!d_a || !d_out || !ext_omega || !zeta || k > ext_k || ext_k > 28 || a_stride < ((size_t)1 << k) || out_stride < ((size_t)1 << ext_k) ||
      a_stride >= ((size_t)1 << 32) || out_stride >= ((size_t)1 << 32)) { set_error("coeff_to_extended: bad argument"); return ZKHIP_EINVAL; }
  if (batch == 0) return ZKHIP_OK;
  uint32_t sc[24];
  coset_scales(zeta, nullptr, sc);
  return device_transform(d_a, 1u << k, a_stride, d_out, 1u << ext_k, out_stride, batch, ext_k, ext_omega, sc, 3, nullptr, 0, stream);
}

int zkhip_extended_to_coeff_device(const void* d_a, size_t a_stride, uint32_t ext_k, const uint64_t ext_omega_inv[4], const uint64_t ext_divisor[4],
                                   const uint64_t zeta[4], void* d_out, size_t out_stride, size_t out_len, uint32_t batch, void* stream) {
  ZK_API_RANGE();
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  if (!d_a || !d_out || !ext_omega_inv || !ext_divisor || !zeta || ext_k > 28 || out_len > ((size_t)1 << ext_k) || a_stride < ((size_t)1 << ext_k) ||
      out_stride < out_len || a_stride >= ((size_t)1 << 32) || out_stride >= ((size_t)1 << 32)) { set_error("extended_to_coeff: bad argument"); return ZKHIP_EINVAL; }
  if (batch == 0 || out_len == 0) return ZKHIP_OK;
  uint32_t sc[24];
  coset_scales(zeta, ext_divisor, sc);
  return device_transform(d_a, 1u << ext_k, a_stride, d_out, (uint32_t)out_len, out_stride, batch, ext_k, ext_omega_inv, nullptr, 0, sc, 3, stream);
}

int zkhip_mul_periodic(uint64_t* a, size_t n, const uint64_t* table, uint32_t period) {
  ZK_API_RANGE();
  if ((n && !a) || !table || period == 0) { set_error("mul_periodic: bad argument"); return ZKHIP_EINVAL; }
  if (n == 0) return ZKHIP_OK;
  lane_hold H;
  if (H.rc != ZKHIP_OK) return H.rc;
  int rc;
  hipStream_t s = H.s;
  if ((rc = H.sc->poly.reserve(n * 32)) != ZKHIP_OK) return rc;
  if ((rc = H.sc->poly2.reserve((size_t)period * 32)) != ZKHIP_OK) return rc;
  HIPCHK(hipMemcpyAsync(H.sc->poly.p, a, n * 32, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(H.sc->poly2.p, table, (size_t)period * 32, hipMemcpyHostToDevice, s));
  if ((rc = fr_mul_periodic_device((uint32_t*)H.sc->poly.p, n, (const uint32_t*)H.sc->poly2.p, period, s)) != ZKHIP_OK) return rc;
  HIPCHK(hipMemcpyAsync(a, H.sc->poly.p, n * 32, hipMemcpyDeviceToHost, s));
  return H.finish();
}

// ---- row a7: Fr-vector primitives ---------------------------------------------------------------------
int zkhip_fr_eval_polynomial_device(const void* d_poly, size_t n, const uint64_t point[4], void* d_out, void* stream) {
  ZK_API_RANGE();
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  if (!point || !d_out || (n && !d_poly)) { set_error("eval_polynomial: null pointer"); return ZKHIP_EINVAL; }
  hipStream_t s = caller_stream(stream);
  scratch* sc = scratch_for(primary(), s);
  if ((rc = sc->ws.reserve(poly_workspace_bytes(n))) != ZKHIP_OK) return rc;
  return fr_eval_polynomial_device((const uint32_t*)d_poly, n, (const uint32_t*)point, (uint32_t*)d_out, sc->ws.p, sc->ws.cap, s);
}

int zkhip_fr_eval_polynomial_batch_device(const void* const* d_polys, size_t count, size_t n, const uint64_t point[4], void* d_out, void* stream) {
  ZK_API_RANGE();
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  if (count && (!d_polys || !point || !d_out)) { set_error("eval_polynomial_batch: null pointer"); return ZKHIP_EINVAL; }
  for (size_t i = 0; i < count && n; i++)
    if (!d_polys[i]) { set_error("eval_polynomial_batch: polynomial %zu is null", i); return ZKHIP_EINVAL; }
  hipStream_t s = caller_stream(stream);
  scratch* sc = scratch_for(primary(), s);
  if ((rc = sc->ws.reserve(poly_batch_workspace_bytes(n, count))) != ZKHIP_OK) return rc;
  return fr_eval_polynomial_batch_device(d_polys, count, n, (const uint32_t*)point, (uint32_t*)d_out, sc->ws.p, sc->ws.cap, s, &sc->args);
}

int zkhip_fr_kate_division_device(const void* d_a, size_t n, const uint64_t b[4], void* d_q, void* stream) {
  ZK_API_RANGE();
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  if (!b || (n > 1 && (!d_a || !d_q))) { set_error("kate_division: null pointer"); return ZKHIP_EINVAL; }
  hipStream_t s = caller_stream(stream);
  scratch* sc = scratch_for(primary(), s);
  if ((rc = sc->ws.reserve(poly_workspace_bytes(n))) != ZKHIP_OK) return rc;
  return fr_kate_division_device((const uint32_t*)d_a, n, (const uint32_t*)b, (uint32_t*)d_q, sc->ws.p, sc->ws.cap, s);
}

// the argument checks of both forms of divide_by_roots: nothing is enqueued before they pass
static int check_roots(const uint64_t* roots, uint32_t m) {
  if (m == 0 || m > ZKHIP_MAX_ROOTS) { set_error("divide_by_roots: %u roots (1 .. %d)", m, ZKHIP_MAX_ROOTS); return ZKHIP_EINVAL; }
  if (!roots) { set_error("divide_by_roots: null pointer"); return ZKHIP_EINVAL; }
  for (uint32_t i = 0; i < m; i++) {
    if (!fr_words_canonical(roots + (size_t)i * 4)) { set_error("divide_by_roots: root %u is not canonical (>= r)", i); return ZKHIP_EINVAL; }
    for (uint32_t j = 0; j < i; j++)
      if (memcmp(roots + i * 4, roots + j * 4, 32) == 0) { set_error("divide_by_roots: roots %u and %u are equal", j, i); return ZKHIP_EINVAL; }
  }
  return ZKHIP_OK;
}

int zkhip_fr_divide_by_roots_device(const void* d_a, size_t n, const uint64_t* roots, uint32_t m, void* d_q, void* d_evals, void* stream) {
  ZK_API_RANGE();
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  if ((rc = check_roots(roots, m)) != ZKHIP_OK) return rc;
  if (n && (!d_a || !d_q)) { set_error("divide_by_roots: null pointer"); return ZKHIP_EINVAL; }
  hipStream_t s = caller_stream(stream);
  scratch* sc = scratch_for(primary(), s);
  if ((rc = sc->ws.reserve(poly_roots_workspace_bytes(n, m))) != ZKHIP_OK) return rc;
  return fr_divide_by_roots_device((const uint32_t*)d_a, n, (const uint32_t(*)[8])roots, m, (uint32_t*)d_q, (uint32_t*)d_evals, sc->ws.p, sc->ws.cap, s);
}

int zkhip_fr_batch_invert_device(void* d_a, size_t n, void* stream) {
  ZK_API_RANGE();
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  if (n && !d_a) { set_error("batch_invert: null pointer"); return ZKHIP_EINVAL; }
  hipStream_t s = caller_stream(stream);
  scratch* sc = scratch_for(primary(), s);
  if ((rc = sc->ws.reserve(poly_workspace_bytes(n))) != ZKHIP_OK) return rc;
  return fr_batch_invert_device((uint32_t*)d_a, n, sc->ws.p, sc->ws.cap, s);
}

int zkhip_fr_prefix_product_device(const void* d_v, size_t n, void* d_out, void* stream) {
  ZK_API_RANGE();
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  if (n && (!d_v || !d_out)) { set_error("prefix_product: null pointer"); return ZKHIP_EINVAL; }
  hipStream_t s = caller_stream(stream);
  scratch* sc = scratch_for(primary(), s);
  if ((rc = sc->ws.reserve(poly_workspace_bytes(n))) != ZKHIP_OK) return rc;
  return fr_prefix_product_device((const uint32_t*)d_v, n, (uint32_t*)d_out, sc->ws.p, sc->ws.cap, s);
}

}  // extern "C"

namespace zkhip {
// host-buffer wrappers: upload to the lane's poly scratch, run on the lane's stream, download
// (`op(d_in, d_out, stream)` is the `_device` call; `in_place`: its result replaces d_in)
template <class Op>
static int host_vec_op(const uint64_t* in, size_t n_in, uint64_t* out, size_t n_out, bool in_place, Op op) {
  lane_hold H;
  if (H.rc != ZKHIP_OK) return H.rc;
  int rc;
  hipStream_t s = H.s;
  if ((rc = H.sc->poly.reserve((n_in + 1) * 32)) != ZKHIP_OK) return rc;
  if ((rc = H.sc->poly2.reserve((n_out + 1) * 32)) != ZKHIP_OK) return rc;
  if (n_in) HIPCHK(hipMemcpyAsync(H.sc->poly.p, in, n_in * 32, hipMemcpyHostToDevice, s));
  if ((rc = op(H.sc->poly.p, H.sc->poly2.p, s)) != ZKHIP_OK) return rc;
  if (n_out) HIPCHK(hipMemcpyAsync(out, in_place ? H.sc->poly.p : H.sc->poly2.p, n_out * 32, hipMemcpyDeviceToHost, s));
  return H.finish();
}
}  // namespace zkhip

extern "C" {

int zkhip_fr_eval_polynomial(const uint64_t* poly, size_t n, const uint64_t point[4], uint64_t out[4]) {
  ZK_API_RANGE();
  if (!point || !out || (n && !poly)) { set_error("eval_polynomial: null pointer"); return ZKHIP_EINVAL; }
  return host_vec_op(poly, n, out, 1, false, [&](void* d_a, void* d_r, void* s) { return zkhip_fr_eval_polynomial_device(d_a, n, point, d_r, s); });
}

int zkhip_fr_kate_division(const uint64_t* a, size_t n, const uint64_t b[4], uint64_t* q) {
  ZK_API_RANGE();
  if (!b || (n > 1 && (!a || !q))) { set_error("kate_division: null pointer"); return ZKHIP_EINVAL; }
  if (n < 2) return ZKHIP_OK;
  return host_vec_op(a, n, q, n - 1, false, [&](void* d_a, void* d_q, void* s) { return zkhip_fr_kate_division_device(d_a, n, b, d_q, s); });
}

int zkhip_fr_divide_by_roots(const uint64_t* a, size_t n, const uint64_t* roots, uint32_t m, uint64_t* q, uint64_t* evals) {
  ZK_API_RANGE();
  int rc = check_roots(roots, m);
  if (rc != ZKHIP_OK) return rc;
  if (n && (!a || !q)) { set_error("divide_by_roots: null pointer"); return ZKHIP_EINVAL; }
  if (n == 0) {
    if (evals) memset(evals, 0, (size_t)m * 32);
    return ZKHIP_OK;
  }
  lane_hold H;
  if (H.rc != ZKHIP_OK) return H.rc;
  hipStream_t s = H.s;
  if ((rc = H.sc->poly.reserve(n * 32)) != ZKHIP_OK) return rc;
  if ((rc = H.sc->poly2.reserve((n + ZKHIP_MAX_ROOTS) * 32)) != ZKHIP_OK) return rc;
  char* d_ev = (char*)H.sc->poly2.p + n * 32;
  HIPCHK(hipMemcpyAsync(H.sc->poly.p, a, n * 32, hipMemcpyHostToDevice, s));
  if ((rc = zkhip_fr_divide_by_roots_device(H.sc->poly.p, n, roots, m, H.sc->poly2.p, evals ? d_ev : nullptr, s)) != ZKHIP_OK) return rc;
  HIPCHK(hipMemcpyAsync(q, H.sc->poly2.p, n * 32, hipMemcpyDeviceToHost, s));
  if (evals) HIPCHK(hipMemcpyAsync(evals, d_ev, (size_t)m * 32, hipMemcpyDeviceToHost, s));
  return H.finish();
}

int zkhip_fr_batch_invert(uint64_t* a, size_t n) {
  ZK_API_RANGE();
  if (n && !a) { set_error("batch_invert: null pointer"); return ZKHIP_EINVAL; }
  if (n == 0) return ZKHIP_OK;
  return host_vec_op(a, n, a, n, true, [&](void* d_a, void*, void* s) { return zkhip_fr_batch_invert_device(d_a, n, s); });
}

int zkhip_fr_prefix_product(const uint64_t* v, size_t n, uint64_t* out) {
  ZK_API_RANGE();
  if (n && (!v || !out)) { set_error("prefix_product: null pointer"); return ZKHIP_EINVAL; }
  if (n == 0) return ZKHIP_OK;
  return host_vec_op(v, n, out, n, false, [&](void* d_v, void* d_out, void* s) { return zkhip_fr_prefix_product_device(d_v, n, d_out, s); });
}

// ---- lookup argument: permute_expression_pair ----------------------------------------------------------------------
int zkhip_lookup_permute_device(const void* d_input, const void* d_table, size_t usable_rows, void* d_permuted_input, void* d_permuted_table,
                                void* stream) {
  ZK_API_RANGE();
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  if (usable_rows && (!d_input || !d_table || !d_permuted_input || !d_permuted_table)) { set_error("lookup_permute: null pointer"); return ZKHIP_EINVAL; }
  if (usable_rows == 0) return ZKHIP_OK;
  hipStream_t s = caller_stream(stream);
  scratch* sc = scratch_for(primary(), s);
  if ((rc = sc->vm.reserve(lookup_permute_workspace_bytes(usable_rows))) != ZKHIP_OK) return rc;
  return lookup_permute_device((const uint32_t*)d_input, (const uint32_t*)d_table, usable_rows, (uint32_t*)d_permuted_input,
                               (uint32_t*)d_permuted_table, sc->vm.p, sc->vm.cap, s);
}

// every argument error of the two many-lookup calls; nothing has been enqueued when it fails
static int lookup_many_args_ok(const char* what, const void* const* d_inputs, const void* const* d_tables, uint32_t n_lookups, uint32_t log_n, size_t usable_rows,
                               bool others_ok) {
  if (!d_inputs || !d_tables || !others_ok) { set_error("%s: null pointer", what); return ZKHIP_EINVAL; }
  if (log_n > 28 || usable_rows > ((size_t)1 << log_n)) { set_error("%s: bad shape (log_n %u, usable_rows %zu)", what, log_n, usable_rows); return ZKHIP_EINVAL; }
  for (uint32_t l = 0; l < n_lookups; l++)
    if (!d_inputs[l] || !d_tables[l]) { set_error("%s: a column of lookup %u is null", what, l); return ZKHIP_EINVAL; }
  return ZKHIP_OK;
}

int zkhip_lookup_permute_many_device(const void* const* d_inputs, const void* const* d_tables, uint32_t n_lookups, uint32_t log_n, size_t usable_rows,
                                     void* d_permuted_inputs, void* d_permuted_tables, void* stream) {
  ZK_API_RANGE();
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  if (n_lookups == 0 || usable_rows == 0) return ZKHIP_OK;
  if ((rc = lookup_many_args_ok("lookup_permute_many", d_inputs, d_tables, n_lookups, log_n, usable_rows, d_permuted_inputs && d_permuted_tables)) != ZKHIP_OK) return rc;
  hipStream_t s = caller_stream(stream);
  scratch* sc = scratch_for(primary(), s);
  if ((rc = sc->vm.reserve(lookup_permute_many_workspace_bytes(n_lookups, usable_rows))) != ZKHIP_OK) return rc;
  return lookup_permute_many_device(d_inputs, d_tables, n_lookups, (size_t)1 << log_n, usable_rows, (uint32_t*)d_permuted_inputs, (uint32_t*)d_permuted_tables,
                                    sc->vm.p, sc->vm.cap, s, &sc->args);
}

int zkhip_lookup_products_device(const void* const* d_inputs, const void* const* d_tables, const void* d_permuted_inputs, const void* d_permuted_tables,
                                 uint32_t n_lookups, uint32_t log_n, size_t usable_rows, const uint64_t beta[4], const uint64_t gamma[4], void* d_z, void* stream) {
  ZK_API_RANGE();
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  if (n_lookups == 0 || usable_rows == 0) return ZKHIP_OK;
  if ((rc = lookup_many_args_ok("lookup_products", d_inputs, d_tables, n_lookups, log_n, usable_rows, d_permuted_inputs && d_permuted_tables && beta && gamma && d_z)) !=
      ZKHIP_OK) return rc;
  hipStream_t s = caller_stream(stream);
  scratch* sc = scratch_for(primary(), s);
  if ((rc = sc->ws.reserve(lookup_products_workspace_bytes(n_lookups, log_n))) != ZKHIP_OK) return rc;
  return fr_lookup_products_device(d_inputs, d_tables, (const uint32_t*)d_permuted_inputs, (const uint32_t*)d_permuted_tables, n_lookups, log_n, usable_rows,
                                   (const uint32_t*)beta, (const uint32_t*)gamma, (uint32_t*)d_z, sc->ws.p, sc->ws.cap, s, &sc->args);
}

// ---- witness checks (include/zkhip.h): gates, copy constraints, lookup membership -----------------------------------------------------------
// Every argument is looked at before anything is enqueued; after that nothing waits for the stream.
static inline bool report_ptr_ok(const void* p) { return p && ((uintptr_t)p & 7u) == 0; }

int zkhip_check_rows_device(const zkhip_vm_program* progs, uint32_t n_progs, const void* const* d_columns, uint32_t n_columns, uint32_t log_rows, uint64_t row0,
                            uint64_t count, void* d_reports, void* stream) {
  ZK_API_RANGE();
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  if (!progs || n_progs == 0 || n_progs > 65535 || !report_ptr_ok(d_reports) || (n_columns && !d_columns)) { set_error("check_rows: bad argument"); return ZKHIP_EINVAL; }
  for (uint32_t p = 0; p < n_progs; p++)
    if ((rc = row_vm_validate(&progs[p], n_columns, log_rows, 0)) != ZKHIP_OK) return rc;
  const uint64_t rows = (uint64_t)1 << log_rows;
  if (count == 0 || count > rows || row0 > rows - count) {
    set_error("check_rows: rows [%llu, +%llu) outside a domain of 2^%u rows", (unsigned long long)row0, (unsigned long long)count, log_rows);
    return ZKHIP_EINVAL;
  }
  for (uint32_t i = 0; i < n_columns; i++)
    if (!d_columns[i]) { set_error("check_rows: column %u is null", i); return ZKHIP_EINVAL; }
  hipStream_t s = caller_stream(stream);
  scratch* sc = scratch_for(primary(), s);
  vm_call c;
  if ((rc = sc->vm_call_for(s, progs, n_progs, d_columns, n_columns, log_rows, &c)) != ZKHIP_OK) return rc;
  c.form = VM_CHECK; c.row0 = row0; c.count = count; c.d_out = (uint32_t*)d_reports;
  return row_vm_launch(c);
}

int zkhip_check_copies_device(const void* const* d_columns, uint32_t n_columns, uint32_t log_n, const void* d_map_col, const void* d_map_row, void* d_report,
                              void* stream) {
  ZK_API_RANGE();
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  if (!d_columns || !d_map_col || !d_map_row || !report_ptr_ok(d_report)) { set_error("check_copies: null pointer"); return ZKHIP_EINVAL; }
  // the column addresses travel through one slot of the argument ring (no wait for the stream), the grid has one lane per cell
  if (n_columns == 0 || (size_t)n_columns * 8 > arg_ring::SLOT_BYTES || log_n > 28 || ((uint64_t)n_columns << log_n) >= (1ull << 39)) {
    set_error("check_copies: bad shape (%u columns of 2^%u rows)", n_columns, log_n);
    return ZKHIP_EINVAL;
  }
  for (uint32_t i = 0; i < n_columns; i++)
    if (!d_columns[i]) { set_error("check_copies: column %u is null", i); return ZKHIP_EINVAL; }
  hipStream_t s = caller_stream(stream);
  scratch* sc = scratch_for(primary(), s);
  if ((rc = sc->ws.reserve((size_t)n_columns * 8)) != ZKHIP_OK) return rc;
  if ((rc = upload_args(&sc->args, sc->ws.p, d_columns, (size_t)n_columns * 8, s)) != ZKHIP_OK) return rc;
  return check_copies_device(sc->ws.p, n_columns, log_n, (const uint32_t*)d_map_col, (const uint32_t*)d_map_row, d_report, s);
}

int zkhip_check_lookups_device(const void* const* d_inputs, const void* const* d_tables, uint32_t n_lookups, uint32_t log_n, size_t usable_rows, void* d_reports,
                               void* stream) {
  ZK_API_RANGE();
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  if (n_lookups == 0) return ZKHIP_OK;
  // the argument block travels through one slot of the argument ring: no wait for the stream
  if (3 * (size_t)n_lookups * 8 > arg_ring::SLOT_BYTES) { set_error("check_lookups: more than %zu lookups", arg_ring::SLOT_BYTES / 24); return ZKHIP_EINVAL; }
  if ((rc = lookup_many_args_ok("check_lookups", d_inputs, d_tables, n_lookups, log_n, usable_rows, report_ptr_ok(d_reports))) != ZKHIP_OK) return rc;
  hipStream_t s = caller_stream(stream);
  scratch* sc = scratch_for(primary(), s);
  if (usable_rows && (rc = sc->vm.reserve(lookup_check_workspace_bytes(n_lookups, usable_rows))) != ZKHIP_OK) return rc;
  return lookup_check_device(d_inputs, d_tables, n_lookups, usable_rows, d_reports, sc->vm.p, sc->vm.cap, s, &sc->args);
}

// ---- the quotient identity at x (include/zkhip.h; verify_identity.hip) ---------------------------------------------------------------------------
// Every refusal is decided before the device is touched (a host without a GPU gets the same ZKHIP_EINVAL); after that nothing waits for the stream.
static inline bool elems_ptr_ok(const void* p) { return p && ((uintptr_t)p & 15u) == 0; }

int zkhip_fr_domain_points_device(uint32_t k, uint32_t usable_rows, const uint64_t omega[4], const void* d_x, size_t n_points, void* d_out, void* stream) {
  ZK_API_RANGE();
  int rc = identity_domain_validate("fr_domain_points", k, usable_rows, omega);
  if (rc != ZKHIP_OK) return rc;
  if (n_points < 1 || n_points > ((size_t)1 << 30)) { set_error("fr_domain_points: %zu points", n_points); return ZKHIP_EINVAL; }
  if (!elems_ptr_ok(d_x) || !elems_ptr_ok(d_out)) { set_error("fr_domain_points: null or misaligned pointer"); return ZKHIP_EINVAL; }
  guard_t g(g_mu);
  if ((rc = ensure_init()) != ZKHIP_OK) return rc;
  return fr_domain_points_device(k, usable_rows, omega, (const uint32_t*)d_x, n_points, (uint32_t*)d_out, caller_stream(stream));
}

// the identity with `lay` resolved (n_queries = 0: no instance columns); `who` names the call in the error text
static int verify_identity_call(const char* who, const zkhip_vm_program* prog, const void* d_evals, uint32_t n_evals, const void* d_challenges, uint32_t k,
                                uint32_t usable_rows, const uint64_t omega[4], const void* d_instances, const instance_layout& lay, size_t n_proofs, void* d_status,
                                void* d_report, void* stream) {
  int rc;
  if (n_proofs > ((size_t)1 << 24)) { set_error("%s: %zu proofs in one call", who, n_proofs); return ZKHIP_EINVAL; }
  const bool arrays_ok = elems_ptr_ok(d_evals) && elems_ptr_ok(d_challenges) && d_status && ((uintptr_t)d_status & 3u) == 0 &&
                         (lay.total_len == 0 || elems_ptr_ok(d_instances));
  if (!report_ptr_ok(d_report) || (n_proofs && !arrays_ok)) {      // (an empty batch names no array)
    set_error("%s: null or misaligned pointer", who);
    return ZKHIP_EINVAL;
  }
  guard_t g(g_mu);
  if ((rc = ensure_init()) != ZKHIP_OK) return rc;
  hipStream_t s = caller_stream(stream);
  scratch* sc = scratch_for(primary(), s);
  if (n_proofs && (rc = sc->poly2.reserve(verify_identity_columns_bytes(n_evals, lay.n_queries, n_proofs))) != ZKHIP_OK) return rc;
  if (n_proofs && (rc = sc->vm.reserve(verify_identity_vm_bytes(prog, n_evals, lay.n_queries))) != ZKHIP_OK) return rc;
  return verify_identity_device(prog, (const uint32_t*)d_evals, n_evals, (const uint32_t*)d_challenges, k, usable_rows, omega, (const uint32_t*)d_instances, lay, n_proofs,
                                (int32_t*)d_status, d_report, sc->poly2.p, sc->vm.p, sc->vm.cap, s, &sc->vm_stage);
}

int zkhip_verify_identity_device(const zkhip_vm_program* prog, const void* d_evals, uint32_t n_evals, const void* d_challenges, uint32_t k, uint32_t usable_rows,
                                 const uint64_t omega[4], size_t n_proofs, void* d_status, void* d_report, void* stream) {
  ZK_API_RANGE();
  if (n_evals == 0) { set_error("verify_identity: no evaluations"); return ZKHIP_EINVAL; }
  int rc = verify_identity_validate(prog, n_evals, 0);
  if (rc != ZKHIP_OK) return rc;
  if ((rc = identity_domain_validate("verify_identity", k, usable_rows, omega)) != ZKHIP_OK) return rc;
  return verify_identity_call("verify_identity", prog, d_evals, n_evals, d_challenges, k, usable_rows, omega, nullptr, instance_layout(), n_proofs, d_status, d_report, stream);
}

int zkhip_verify_identity_instances_device(const zkhip_vm_program* prog, const void* d_evals, uint32_t n_evals, const void* d_challenges, uint32_t k, uint32_t usable_rows,
                                           const uint64_t omega[4], const void* d_instances, const uint32_t* column_lens, uint32_t n_columns,
                                           const uint32_t* query_columns, const uint32_t* query_rotations, uint32_t n_queries, size_t n_proofs, void* d_status,
                                           void* d_report, void* stream) {
  ZK_API_RANGE();
  const char* who = "verify_identity_instances";
  if (n_evals == 0) { set_error("%s: no evaluations", who); return ZKHIP_EINVAL; }
  if (n_columns > INSTANCE_MAX_QUERIES || n_queries > INSTANCE_MAX_QUERIES) {
    set_error("%s: %u instance columns, %u queries: at most %u of each", who, n_columns, n_queries, INSTANCE_MAX_QUERIES);
    return ZKHIP_EINVAL;
  }
  int rc = verify_identity_validate(prog, n_evals, n_queries);
  if (rc != ZKHIP_OK) return rc;
  if ((rc = identity_domain_validate(who, k, usable_rows, omega)) != ZKHIP_OK) return rc;
  instance_layout lay;                                             // the three host arrays are consumed here
  if ((rc = instance_queries_validate(who, k, usable_rows, "usable_rows", column_lens, n_columns, query_columns, query_rotations, n_queries, &lay)) != ZKHIP_OK) return rc;
  return verify_identity_call(who, prog, d_evals, n_evals, d_challenges, k, usable_rows, omega, d_instances, lay, n_proofs, d_status, d_report, stream);
}

int zkhip_fr_instance_evals_device(uint32_t k, const uint64_t omega[4], const void* d_x, const void* d_instances, const uint32_t* column_lens, uint32_t n_columns,
                                   const uint32_t* query_columns, const uint32_t* query_rotations, uint32_t n_queries, size_t n_proofs, void* d_out, void* stream) {
  ZK_API_RANGE();
  const char* who = "fr_instance_evals";
  if (k < 1) { set_error("%s: k = 0", who); return ZKHIP_EINVAL; }
  int rc = identity_domain_validate(who, k, k <= 28 ? ((uint64_t)1 << k) - 1 : 1, omega);      // k and omega; the call has no usable_rows: 2^k - 1 is valid for every k
  if (rc != ZKHIP_OK) return rc;
  instance_layout lay;
  if ((rc = instance_queries_validate(who, k, (uint64_t)1 << k, "2^k", column_lens, n_columns, query_columns, query_rotations, n_queries, &lay)) != ZKHIP_OK) return rc;
  if (n_proofs > ((size_t)1 << 24)) { set_error("%s: %zu proofs in one call", who, n_proofs); return ZKHIP_EINVAL; }
  if (n_proofs && ((n_queries && (!elems_ptr_ok(d_x) || !elems_ptr_ok(d_out))) || (lay.total_len && !elems_ptr_ok(d_instances)))) {
    set_error("%s: null or misaligned pointer", who);
    return ZKHIP_EINVAL;
  }
  if (n_proofs == 0 || n_queries == 0) return ZKHIP_OK;            // nothing to write
  guard_t g(g_mu);
  if ((rc = ensure_init()) != ZKHIP_OK) return rc;
  return fr_instance_evals_device(k, omega, (const uint32_t*)d_x, (const uint32_t*)d_instances, lay, n_proofs, (uint32_t*)d_out, caller_stream(stream));
}

// ---- the batch verifier's scalar side (include/zkhip.h; gwc_fold.hip): refusals before the device is touched, then nothing waits for the stream ----
int zkhip_gwc_scalars_device(const zkhip_gwc_plan* plan, const void* d_evals, const void* d_points, uint32_t k, const uint64_t omega[4], size_t n_proofs,
                             void* d_rows_a, void* d_rows_c, void* stream) {
  ZK_API_RANGE();
  int rc = gwc_plan_validate(plan, k, omega);
  if (rc != ZKHIP_OK) return rc;
  if (n_proofs > ((size_t)1 << 24)) { set_error("gwc_scalars: %zu proofs in one call", n_proofs); return ZKHIP_EINVAL; }
  if (n_proofs == 0) return ZKHIP_OK;                                // nothing to write
  if (!elems_ptr_ok(d_evals) || !elems_ptr_ok(d_points) || !elems_ptr_ok(d_rows_a) || !elems_ptr_ok(d_rows_c)) {
    set_error("gwc_scalars: null or misaligned pointer");
    return ZKHIP_EINVAL;
  }
  guard_t g(g_mu);
  if ((rc = ensure_init()) != ZKHIP_OK) return rc;
  hipStream_t s = caller_stream(stream);
  scratch* sc = scratch_for(primary(), s);
  if ((rc = sc->ws.reserve(gwc_scalars_workspace_bytes(plan))) != ZKHIP_OK) return rc;
  return gwc_scalars_device(plan, (const uint32_t*)d_evals, (const uint32_t*)d_points, k, omega, n_proofs, (uint32_t*)d_rows_a, (uint32_t*)d_rows_c, sc->ws.p, sc->ws.cap, s,
                            &sc->args);
}

int zkhip_fr_fold_rows_device(const void* d_rows, uint32_t n_cols, uint32_t n_own, const void* d_r, int negate, size_t n_rows, void* d_out_own, void* d_out_shared,
                              void* stream) {
  ZK_API_RANGE();
  const char* who = "fr_fold_rows";
  if (n_cols < 1 || n_cols > 65536 || n_own > n_cols) { set_error("%s: n_cols = %u (1 .. 65536), n_own = %u", who, n_cols, n_own); return ZKHIP_EINVAL; }
  if (negate != 0 && negate != 1) { set_error("%s: negate = %d", who, negate); return ZKHIP_EINVAL; }
  if (n_rows > ((size_t)1 << 24) || (uint64_t)n_rows * n_cols > ((uint64_t)1 << 32)) { set_error("%s: %zu rows of %u columns", who, n_rows, n_cols); return ZKHIP_EINVAL; }
  const uint32_t n_shared = n_cols - n_own;
  if ((n_rows && (!elems_ptr_ok(d_rows) || !elems_ptr_ok(d_r) || (n_own && !elems_ptr_ok(d_out_own)))) || (n_shared && !elems_ptr_ok(d_out_shared))) {
    set_error("%s: null or misaligned pointer", who);
    return ZKHIP_EINVAL;
  }
  if (n_rows == 0 && n_shared == 0) return ZKHIP_OK;                 // nothing to write
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  hipStream_t s = caller_stream(stream);
  scratch* sc = scratch_for(primary(), s);
  if ((rc = sc->ws.reserve(fold_rows_workspace_bytes(n_cols, n_own, n_rows))) != ZKHIP_OK) return rc;
  return fold_rows_device((const uint32_t*)d_rows, n_cols, n_own, (const uint32_t*)d_r, (uint32_t)negate, n_rows, (uint32_t*)d_out_own, (uint32_t*)d_out_shared, sc->ws.p,
                          sc->ws.cap, s);
}

int zkhip_shplonk_scalars_device(const zkhip_shplonk_plan* plan, const void* d_evals, const void* d_points, uint32_t k, const uint64_t omega[4], size_t n_proofs,
                                 void* d_rows_a, void* d_rows_c, void* d_status, void* stream) {
  ZK_API_RANGE();
  std::vector<uint32_t> blob;
  int rc = shplonk_plan_marshal(plan, k, omega, &blob);
  if (rc != ZKHIP_OK) return rc;
  if (n_proofs > ((size_t)1 << 24)) { set_error("shplonk_scalars: %zu proofs in one call", n_proofs); return ZKHIP_EINVAL; }
  if (n_proofs == 0) return ZKHIP_OK;                                // nothing to write
  if (!elems_ptr_ok(d_evals) || !elems_ptr_ok(d_points) || !elems_ptr_ok(d_rows_a) || !elems_ptr_ok(d_rows_c) || !elems_ptr_ok(d_status)) {
    set_error("shplonk_scalars: null or misaligned pointer");
    return ZKHIP_EINVAL;
  }
  guard_t g(g_mu);
  if ((rc = ensure_init()) != ZKHIP_OK) return rc;
  hipStream_t s = caller_stream(stream);
  scratch* sc = scratch_for(primary(), s);
  if ((rc = sc->ws.reserve(blob.size() * 4)) != ZKHIP_OK) return rc;
  return shplonk_scalars_device(blob, (const uint32_t*)d_evals, (const uint32_t*)d_points, n_proofs, (uint32_t*)d_rows_a, (uint32_t*)d_rows_c, (uint32_t*)d_status, sc->ws.p,
                                sc->ws.cap, s, &sc->args);
}

// ---- KZG accumulators (include/zkhip.h; row_msm.hip, row_msm.hpp, kzg_limbs.hpp): refusals before the device is touched, nothing waits for the stream ----
int zkhip_g1_row_msm_device(const void* d_rows, size_t n_cols, const void* d_own_points, size_t n_own, size_t own_stride, const void* d_shared_points, size_t n_rows,
                            void* d_out_xyz, void* stream) {
  ZK_API_RANGE();
  if (const char* why = row_msm_refusal(d_rows, n_cols, d_own_points, n_own, own_stride, d_shared_points, n_rows, d_out_xyz)) {
    set_error("g1_row_msm: %s (%zu rows of %zu columns, %zu own at stride %zu)", why, n_rows, n_cols, n_own, own_stride);
    return ZKHIP_EINVAL;
  }
  if (n_rows == 0) return ZKHIP_OK;                                  // nothing to write
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  hipStream_t s = caller_stream(stream);
  scratch* sc = scratch_for(primary(), s);
  if ((rc = sc->ws.reserve(g1_row_msm_workspace(n_rows, n_cols))) != ZKHIP_OK) return rc;
  return g1_row_msm_device((const uint32_t*)d_rows, n_cols, (const uint32_t*)d_own_points, n_own, own_stride, (const uint32_t*)d_shared_points, n_rows, (uint32_t*)d_out_xyz,
                           sc->ws.p, sc->ws.cap, s);
}

int zkhip_kzg_limbs_encode(const uint64_t* affine, size_t n, uint64_t* fr_out) {
  if (n && (!affine || !fr_out)) { set_error("kzg_limbs_encode: null pointer"); return ZKHIP_EINVAL; }
  for (size_t i = 0; i < n; i++) kzg_limbs::encode_point(affine + i * 8, fr_out + i * 24);
  return ZKHIP_OK;
}

int zkhip_kzg_limbs_decode(const uint64_t* fr_in, size_t n, uint64_t* affine, uint32_t* status) {
  if (n && (!fr_in || !affine || !status)) { set_error("kzg_limbs_decode: null pointer"); return ZKHIP_EINVAL; }
  for (size_t i = 0; i < n; i++) status[i] = kzg_limbs::decode_point(fr_in + i * 24, affine + i * 8);
  return ZKHIP_OK;
}

int zkhip_kzg_limbs_encode_device(const void* d_affine, size_t n, void* d_fr_out, void* stream) {
  ZK_API_RANGE();
  if (n > ((size_t)1 << 31)) { set_error("kzg_limbs_encode: %zu points in one call", n); return ZKHIP_EINVAL; }
  if (n && (!elems_ptr_ok(d_affine) || !elems_ptr_ok(d_fr_out))) { set_error("kzg_limbs_encode: null or misaligned pointer"); return ZKHIP_EINVAL; }
  if (n == 0) return ZKHIP_OK;
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  return kzg_limbs_encode_device((const uint64_t*)d_affine, n, (uint64_t*)d_fr_out, caller_stream(stream));
}

int zkhip_kzg_limbs_decode_device(const void* d_fr_in, size_t n, void* d_affine, void* d_status, void* stream) {
  ZK_API_RANGE();
  if (n > ((size_t)1 << 31)) { set_error("kzg_limbs_decode: %zu points in one call", n); return ZKHIP_EINVAL; }
  if (n && (!elems_ptr_ok(d_fr_in) || !elems_ptr_ok(d_affine) || !d_status || ((uintptr_t)d_status & 3u) != 0)) {
    set_error("kzg_limbs_decode: null or misaligned pointer");
    return ZKHIP_EINVAL;
  }
  if (n == 0) return ZKHIP_OK;
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  return kzg_limbs_decode_device((const uint64_t*)d_fr_in, n, (uint64_t*)d_affine, (uint32_t*)d_status, caller_stream(stream));
}

int zkhip_lookup_permute(const uint64_t* input, const uint64_t* table, size_t usable_rows, uint64_t* permuted_input, uint64_t* permuted_table) {
  ZK_API_RANGE();
  if (usable_rows && (!input || !table || !permuted_input || !permuted_table)) { set_error("lookup_permute: null pointer"); return ZKHIP_EINVAL; }
  if (usable_rows == 0) return ZKHIP_OK;
  lane_hold H;
  if (H.rc != ZKHIP_OK) return H.rc;
  int rc;
  const size_t bytes = usable_rows * 32;
  hipStream_t s = H.s;
  if ((rc = H.sc->poly.reserve(2 * bytes)) != ZKHIP_OK) return rc;
  if ((rc = H.sc->poly2.reserve(2 * bytes)) != ZKHIP_OK) return rc;
  char* in = (char*)H.sc->poly.p;
  char* out = (char*)H.sc->poly2.p;
  HIPCHK(hipMemcpyAsync(in, input, bytes, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(in + bytes, table, bytes, hipMemcpyHostToDevice, s));
  if ((rc = zkhip_lookup_permute_device(in, in + bytes, usable_rows, out, out + bytes, s)) != ZKHIP_OK) return rc;
  HIPCHK(hipMemcpyAsync(permuted_input, out, bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(permuted_table, out + bytes, bytes, hipMemcpyDeviceToHost, s));
  return H.finish();
}

// ---- random field elements (fr_random.hpp, random.hip) ---------------------------------------------------------------
// first + count > 2^64: the stream has no such index
static inline bool random_range_ok(uint64_t first, uint64_t count) { return first == 0 || count <= (uint64_t)0 - first; }

int zkhip_fr_random_device(const uint8_t seed[32], uint64_t stream_id, uint64_t first, size_t n, void* d_out, void* stream) {
  ZK_API_RANGE();
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  if (n == 0) return ZKHIP_OK;
  if (!seed || !d_out) { set_error("fr_random: null pointer"); return ZKHIP_EINVAL; }
  if (!random_range_ok(first, n)) { set_error("fr_random: first + n exceeds 2^64"); return ZKHIP_EINVAL; }
  return fr_random_device(seed, stream_id, first, n, (uint32_t*)d_out, caller_stream(stream));
}

int zkhip_fr_random_rows_device(const uint8_t seed[32], uint64_t stream_id, uint64_t first, const void* const* d_cols, uint32_t n_cols, size_t row0, size_t count,
                                void* stream) {
  ZK_API_RANGE();
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  if (n_cols == 0 || count == 0) return ZKHIP_OK;
  if (!seed || !d_cols) { set_error("fr_random_rows: null pointer"); return ZKHIP_EINVAL; }
  for (uint32_t c = 0; c < n_cols; c++)
    if (!d_cols[c]) { set_error("fr_random_rows: column %u is null", c); return ZKHIP_EINVAL; }
  if (count > ((size_t)1 << 30) / n_cols) { set_error("fr_random_rows: %u columns x %zu rows exceed 2^30 elements", n_cols, count); return ZKHIP_EINVAL; }
  if (!random_range_ok(first, (uint64_t)n_cols * count)) { set_error("fr_random_rows: first + n_cols * count exceeds 2^64"); return ZKHIP_EINVAL; }
  hipStream_t s = caller_stream(stream);
  scratch* sc = scratch_for(primary(), s);
  if ((rc = sc->ws.reserve(fr_random_rows_workspace_bytes(n_cols))) != ZKHIP_OK) return rc;
  return fr_random_rows_device(seed, stream_id, first, d_cols, n_cols, row0, count, sc->ws.p, sc->ws.cap, s, &sc->args);
}

int zkhip_fr_random(const uint8_t seed[32], uint64_t stream_id, uint64_t first, size_t n, uint64_t* out) {
  ZK_API_RANGE();
  if (n == 0) return ZKHIP_OK;
  if (!seed || !out) { set_error("fr_random: null pointer"); return ZKHIP_EINVAL; }
  return host_vec_op(nullptr, 0, out, n, false, [&](void*, void* d_out, void* s) { return zkhip_fr_random_device(seed, stream_id, first, n, d_out, s); });
}

// ---- device buffers for hosts that do not link HIP -------------------------------------------------------------
int zkhip_alloc(size_t bytes, void** d_ptr) {
  ZK_API_RANGE();
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  if (!d_ptr) { set_error("alloc: null pointer"); return ZKHIP_EINVAL; }
  *d_ptr = nullptr;
  if (bytes == 0) return ZKHIP_OK;
  if (hipMalloc(d_ptr, bytes) != hipSuccess) { (void)hipGetLastError(); *d_ptr = nullptr; set_error("hipMalloc(%zu) failed", bytes); return ZKHIP_ENOMEM; }
  return ZKHIP_OK;
}

int zkhip_free(void* d_ptr) {
  ZK_API_RANGE();
  guard_t g(g_mu);
  if (!d_ptr) return ZKHIP_OK;
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  HIPCHK(hipDeviceSynchronize());               // kernels queued on any stream may still use it
  HIPCHK(hipFree(d_ptr));
  return ZKHIP_OK;
}

int zkhip_upload(void* d_dst, const void* src, size_t bytes) {
  ZK_API_RANGE();
  { guard_t g(g_mu); int rc = ensure_init(); if (rc != ZKHIP_OK) return rc; }
  if (bytes && (!d_dst || !src)) { set_error("upload: null pointer"); return ZKHIP_EINVAL; }
  if (bytes == 0) return ZKHIP_OK;
  HIPCHK(hipMemcpy(d_dst, src, bytes, hipMemcpyHostToDevice));      // default stream, blocking
  return ZKHIP_OK;
}

int zkhip_download(void* dst, const void* d_src, size_t bytes) {
  ZK_API_RANGE();
  { guard_t g(g_mu); int rc = ensure_init(); if (rc != ZKHIP_OK) return rc; }
  if (bytes && (!dst || !d_src)) { set_error("download: null pointer"); return ZKHIP_EINVAL; }
  if (bytes == 0) return ZKHIP_OK;
  HIPCHK(hipMemcpy(dst, d_src, bytes, hipMemcpyDeviceToHost));
  return ZKHIP_OK;
}

int zkhip_stream_sync(void* stream) {
  ZK_API_RANGE();
  { guard_t g(g_mu); int rc = ensure_init(); if (rc != ZKHIP_OK) return rc; }
  HIPCHK(hipStreamSynchronize(caller_stream(stream)));
  return ZKHIP_OK;
}

int zkhip_sync(void) {
  ZK_API_RANGE();
  { guard_t g(g_mu); int rc = ensure_init(); if (rc != ZKHIP_OK) return rc; }
  HIPCHK(hipDeviceSynchronize());
  return ZKHIP_OK;
}

// ---- section 8(f): row programs and grand products -------------------------------------------------------------
int zkhip_fr_eval_rows_device(const zkhip_vm_program* prog, const void* const* d_columns, uint32_t n_columns, uint32_t log_rows,
                              int accumulate, void* d_out, void* stream) {
  ZK_API_RANGE();
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  if ((rc = row_vm_validate(prog, n_columns, log_rows, accumulate)) != ZKHIP_OK) return rc;
  if (!d_out || (n_columns && !d_columns)) { set_error("eval_rows: null pointer"); return ZKHIP_EINVAL; }
  hipStream_t s = caller_stream(stream);
  scratch* sc = scratch_for(primary(), s);
  vm_call c;
  if ((rc = sc->vm_call_for(s, prog, 1, d_columns, n_columns, log_rows, &c)) != ZKHIP_OK) return rc;
  c.accumulate = accumulate; c.d_out = (uint32_t*)d_out;
  return row_vm_launch(c);
}

// out[row] = sum_p weights[p] * progs[p](row): independent row programs over the same columns in ONE launch (blockIdx.y = program:
// vm_call::d_outs), their outputs combined by the linear-combination kernel.  What it is for: the quotient numerator of a circuit with
// hundreds of columns at 2^13 .. 2^15 rows is thousands of instructions over a few thousand rows -- one program is a handful of wavefronts
// walking the whole list.  (Separate launches on side streams overlapped four at a time -- the hardware queues: 2.3 x where one grid gives 8 x.)
int zkhip_fr_eval_rows_sum_device(const zkhip_vm_program* progs, const uint64_t* weights, uint32_t n_progs, const void* const* d_columns, uint32_t n_columns,
                                  uint32_t log_rows, void* d_out, void* stream) {
  ZK_API_RANGE();
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  if (!progs || !weights || n_progs == 0 || n_progs > 4096 || !d_out || (n_columns && !d_columns)) { set_error("eval_rows_sum: bad argument"); return ZKHIP_EINVAL; }
  for (uint32_t p = 0; p < n_progs; p++)
    if ((rc = row_vm_validate(&progs[p], n_columns, log_rows, 0)) != ZKHIP_OK) return rc;
  hipStream_t s = caller_stream(stream);
  scratch* sc = scratch_for(primary(), s);
  const size_t rows = (size_t)1 << log_rows;
  if ((rc = sc->poly2.reserve((size_t)n_progs * rows * 32)) != ZKHIP_OK) return rc;
  vm_call c;
  if ((rc = sc->vm_call_for(s, progs, n_progs, d_columns, n_columns, log_rows, &c)) != ZKHIP_OK) return rc;
  std::vector<uint32_t*> partial(n_progs);
  for (uint32_t p = 0; p < n_progs; p++) partial[p] = (uint32_t*)((char*)sc->poly2.p + (size_t)p * rows * 32);
  c.d_outs = partial.data();
  if ((rc = row_vm_launch(c)) != ZKHIP_OK) return rc;
  if ((rc = sc->ws.reserve(lincomb_workspace_bytes(n_progs, rows))) != ZKHIP_OK) return rc;
  return fr_linear_combination_device((const void* const*)partial.data(), (const uint32_t*)weights, n_progs, rows, (uint32_t*)d_out, sc->ws.p, sc->ws.cap, s, &sc->args);
}

// Row program over window buffers: `count` rows from global row `row0` of a 2^log_rows domain (include/zkhip.h; VM_WINDOW of rowvm.hip)
int zkhip_fr_eval_rows_window_device(const zkhip_vm_program* prog, const void* const* d_windows, uint32_t n_columns, uint32_t log_rows, uint64_t row0,
                                     uint64_t count, int accumulate, void* d_out, void* stream) {
  ZK_API_RANGE();
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  if ((rc = row_vm_validate(prog, n_columns, log_rows, accumulate)) != ZKHIP_OK) return rc;
  if (!d_out || (n_columns && !d_windows)) { set_error("eval_rows_window: null pointer"); return ZKHIP_EINVAL; }
  const uint64_t rows = (uint64_t)1 << log_rows;
  if (row0 >= rows || count == 0 || count > rows) { set_error("eval_rows_window: row0 %llu / count %llu outside a domain of 2^%u rows", (unsigned long long)row0,
                                                              (unsigned long long)count, log_rows); return ZKHIP_EINVAL; }
  for (uint32_t i = 0; i < n_columns; i++)
    if (!d_windows[i]) { set_error("eval_rows_window: window %u is null", i); return ZKHIP_EINVAL; }
  uint64_t lo = 0, hi = 0;
  row_vm_halos(prog, &lo, &hi);
  if (lo + hi >= ((uint64_t)1 << 31)) { set_error("eval_rows_window: halos %llu + %llu too wide", (unsigned long long)lo, (unsigned long long)hi); return ZKHIP_EINVAL; }
  hipStream_t s = caller_stream(stream);
  scratch* sc = scratch_for(primary(), s);
  vm_call c;
  if ((rc = sc->vm_call_for(s, prog, 1, d_windows, n_columns, log_rows, &c)) != ZKHIP_OK) return rc;
  c.form = VM_WINDOW; c.row0 = row0; c.count = count; c.accumulate = accumulate; c.d_out = (uint32_t*)d_out;
  return row_vm_launch(c);
}

// The quotient numerator re-cut by rows over the devices of zkhip_init.  Device j of S: rows shard_range(2^ext_k, j, S),
// COEFF columns shard_range(n_coeff, j, S) in argument order.  Steps, all enqueued from this thread (nothing here waits for a device):
//   A  every device's stream waits for the caller's stream (fan_call's entry event) and for the previous call's last steps on every device
//      (its transforms overwrite q_ext, which the previous call's window copies read);
//   B  each owner pulls its COEFF columns from the primary and runs coeff_to_extended into q_ext (its own twiddle plan), records q_transformed;
//   C  device j waits for every owner's q_transformed, fills its window buffers with peer copies (COEFF columns from their owner's q_ext,
//      EXTENDED columns from the primary), runs the window kernel and copies its `count` results into d_out;
//   D  the caller's stream waits for every device's q_done.
// S = 1 is the composition itself: the transforms into the caller stream's scratch set and the whole-domain launch, no window copies.  The result is the same bytes for
// every S: each transform runs on one device, each row's program reads the same values.
int zkhip_fr_eval_rows_sharded_device(const zkhip_vm_program* prog, const void* const* d_columns, const uint32_t* forms, uint32_t n_columns, uint32_t k,
                                      uint32_t ext_k, const uint64_t ext_omega[4], const uint64_t zeta[4], void* d_out, void* stream) {
  ZK_API_RANGE();
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  if (!prog || !d_out || !ext_omega || !zeta || (n_columns && (!d_columns || !forms))) { set_error("eval_rows_sharded: null pointer"); return ZKHIP_EINVAL; }
  if (k > ext_k || ext_k > 28) { set_error("eval_rows_sharded: k = %u, ext_k = %u out of range", k, ext_k); return ZKHIP_EINVAL; }
  if ((rc = row_vm_validate(prog, n_columns, ext_k, 0)) != ZKHIP_OK) return rc;
  uint64_t halo_lo = 0, halo_hi = 0;
  row_vm_halos(prog, &halo_lo, &halo_hi);
  if (halo_lo + halo_hi >= ((uint64_t)1 << 31)) { set_error("eval_rows_sharded: halos too wide"); return ZKHIP_EINVAL; }
  std::vector<uint32_t> coeff_cols;                        // argument indices of the COEFF columns
  std::vector<const row_shards_t*> rs_set(n_columns, nullptr);   // ZKHIP_COL_ROW_SHARDS columns: the set and column behind the reference
  std::vector<uint32_t> rs_col(n_columns, 0);
  uint32_t n_copied = 0;                                   // columns whose windows this call fills (COEFF and EXTENDED)
  for (uint32_t i = 0; i < n_columns; i++) {
    if (!d_columns[i]) { set_error("eval_rows_sharded: column %u is null", i); return ZKHIP_EINVAL; }
    if (forms[i] > ZKHIP_COL_ROW_SHARDS) { set_error("eval_rows_sharded: column %u has form %u", i, forms[i]); return ZKHIP_EINVAL; }
    if (forms[i] == ZKHIP_COL_COEFF) coeff_cols.push_back(i);
    if (forms[i] != ZKHIP_COL_ROW_SHARDS) { n_copied++; continue; }
    // the reference is a host struct: a device address here is a caller's mistake, refused before anything reads it
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, d_columns[i]) == hipSuccess && (attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeArray)) {
      set_error("eval_rows_sharded: column %u has form ZKHIP_COL_ROW_SHARDS but a device address (a zkhip_row_shard_ref is host memory)", i);
      return ZKHIP_EINVAL;
    }
    (void)hipGetLastError();
    const zkhip_row_shard_ref ref = *(const zkhip_row_shard_ref*)d_columns[i];
    const row_shards_t* R = find_row_shards(ref.set, "eval_rows_sharded");
    if (!R) return ZKHIP_EINVAL;
    if (ref.col >= R->n_cols || R->ext_k != ext_k || R->halo_lo < halo_lo || R->halo_hi < halo_hi) {
      set_error("eval_rows_sharded: column %u: set column %u of %u, ext_k %u (call %u), halos %llu / %llu (program %llu / %llu)", i, ref.col, R->n_cols, R->ext_k,
                ext_k, (unsigned long long)R->halo_lo, (unsigned long long)R->halo_hi, (unsigned long long)halo_lo, (unsigned long long)halo_hi);
      return ZKHIP_EINVAL;
    }
    rs_set[i] = R;
    rs_col[i] = ref.col;
  }
  // device j's window of a ZKHIP_COL_ROW_SHARDS column in the program's halos; the set's event on (j, stream) follows the launch that reads it
  auto rs_window = [&](int j, uint32_t c) -> const void* { return rs_set[c]->window(j, rs_col[c]) + (rs_set[c]->halo_lo - halo_lo) * 8; };
  auto rs_touch = [&](int j, hipStream_t st) -> int {
    for (uint32_t c = 0; c < n_columns; c++)
      if (rs_set[c]) { int r = touch_row_shards(const_cast<row_shards_t*>(rs_set[c]), j, st); if (r != ZKHIP_OK) return r; }
    return ZKHIP_OK;
  };
  hipStream_t s = caller_stream(stream);
  const int S = (int)g_ctx.devs.size();
  const size_t N = (size_t)1 << ext_k, n_in = (size_t)1 << k, nC = coeff_cols.size();
  uint32_t scales[24];
  coset_scales(zeta, nullptr, scales);
  device_ctx& P = primary();
  scratch* sc = scratch_for(P, s);
  prof_begin(s);
  if (S == 1) {
    // the cosets go to the caller stream's scratch set: calls on other streams have sets of their own, calls on this one are ordered by it
    if ((rc = sc->q_ext.reserve(std::max<size_t>(nC, 1) * N * 32)) != ZKHIP_OK) return rc;
    std::vector<const void*> cols(d_columns, d_columns + n_columns);
    for (uint32_t c = 0; c < n_columns; c++)
      if (rs_set[c]) cols[c] = rs_set[c]->window(0, rs_col[c]) + rs_set[c]->halo_lo * 8;   // the whole column sits behind the set's halo_lo
    {
      prof_hold hold;
      for (size_t c = 0; c < nC; c++) {
        uint32_t* dst = (uint32_t*)sc->q_ext.p + c * N * 8;
        if ((rc = run_transform(sc, (const uint32_t*)d_columns[coeff_cols[c]], (uint32_t)n_in, (uint32_t)n_in, dst, (uint32_t)N, (uint32_t)N, 1, ext_k,
                                (const uint32_t*)ext_omega, scales, 3, nullptr, 0, s)) != ZKHIP_OK) return rc;
        cols[coeff_cols[c]] = dst;
      }
    }
    prof_mark(s, "transform");
    prof_mark(s, "exchange");                              // (empty on one device: the same four phases for every S)
    int compiled = 0;
    vm_call c;
    if ((rc = sc->vm_call_for(s, prog, 1, cols.data(), n_columns, ext_k, &c)) != ZKHIP_OK) return rc;
    c.d_out = (uint32_t*)d_out; c.compiled = &compiled;
    if ((rc = row_vm_launch(c)) != ZKHIP_OK) return rc;
    if ((rc = rs_touch(0, s)) != ZKHIP_OK) return rc;
    prof_mark(s, compiled ? "rows_compiled" : "rows_interpreted");
    prof_mark(s, "gather");
    return ZKHIP_OK;
  }
  std::unique_lock<std::mutex> fan(g_fanout_mu);
  std::vector<scratch*> dsc(S, nullptr);
  std::vector<size_t> row_lo(S), row_n(S), own_lo(S), own_n(S);
  // A: streams, scratch, events; every device's first step waits for the entry event and for the previous call's last steps
  bool grows = false;
  for (int j = 0; j < S; j++) {
    device_ctx* D = g_ctx.devs[(size_t)j];
    size_t lo, hi, olo, ohi;
    shard_range(N, j, S, &lo, &hi);
    shard_range(nC, j, S, &olo, &ohi);
    grows |= D->q_ext.cap < std::max<size_t>(ohi - olo, 1) * N * 32 || D->q_win.cap < std::max<size_t>(n_copied, 1) * (halo_lo + hi - lo + halo_hi) * 32 ||
             (j > 0 && D->q_out.cap < std::max<size_t>(hi - lo, 1) * 32);
  }
  // a buffer about to be replaced may still be read by another device's copies of the previous call: the ONE place this call blocks the host
  // thread, and only when a shape needs more scratch than any earlier call (a second call of the same shape allocates nothing and never waits)
  if (grows)
    for (auto* D : g_ctx.devs) if (D->q_done_live) HIPCHK(hipEventSynchronize(D->q_done));
  fan_call F;                                              // an error return from here on waits for every device's stream
  if ((rc = F.begin(s)) != ZKHIP_OK) return rc;
  const std::vector<hipStream_t>& st = F.st;               // the stream device j works on: the caller's for the primary, its fan stream otherwise
  for (int j = 0; j < S; j++) {
    device_ctx* D = g_ctx.devs[(size_t)j];
    if ((rc = F.dev(j)) != ZKHIP_OK) return rc;
    if (!D->q_transformed) HIPCHK(hipEventCreateWithFlags(&D->q_transformed, hipEventDisableTiming));
    if (!D->q_done) HIPCHK(hipEventCreateWithFlags(&D->q_done, hipEventDisableTiming));
    dsc[j] = scratch_for(*D, st[j]);
    shard_range(N, j, S, &row_lo[j], &row_n[j]);
    row_n[j] -= row_lo[j];
    shard_range(nC, j, S, &own_lo[j], &own_n[j]);
    own_n[j] -= own_lo[j];
    const size_t W = halo_lo + row_n[j] + halo_hi;
    if ((rc = D->q_ext.reserve(std::max<size_t>(own_n[j], 1) * N * 32)) != ZKHIP_OK) return rc;
    if ((rc = D->q_win.reserve(std::max<size_t>(n_copied, 1) * W * 32)) != ZKHIP_OK) return rc;
    if (j > 0 && (rc = D->q_out.reserve(std::max<size_t>(row_n[j], 1) * 32)) != ZKHIP_OK) return rc;
    if ((rc = dsc[j]->vm.reserve(row_vm_workspace_bytes(prog, 1, n_columns, ext_k))) != ZKHIP_OK) return rc;
  }
  for (int j = 0; j < S; j++) {
    if ((rc = F.dev(j)) != ZKHIP_OK) return rc;
    for (int i = 0; i < S; i++)
      if (g_ctx.devs[(size_t)i]->q_done_live) HIPCHK(hipStreamWaitEvent(st[j], g_ctx.devs[(size_t)i]->q_done, 0));
  }
  // B: the transforms, each on its owner
  for (int j = 0; j < S; j++) {
    device_ctx* D = g_ctx.devs[(size_t)j];
    if ((rc = F.dev(j)) != ZKHIP_OK) return rc;
    prof_hold hold;
    uint32_t* ext = (uint32_t*)D->q_ext.p;
    for (size_t c = 0; c < own_n[j]; c++) {
      const uint32_t* src = (const uint32_t*)d_columns[coeff_cols[own_lo[j] + c]];
      if (j == 0) {
        if ((rc = run_transform(dsc[j], src, (uint32_t)n_in, (uint32_t)n_in, ext + c * N * 8, (uint32_t)N, (uint32_t)N, 1, ext_k, (const uint32_t*)ext_omega, scales, 3,
                                nullptr, 0, st[j])) != ZKHIP_OK) return rc;
      } else {
        HIPCHK(hipMemcpyPeerAsync(ext + c * N * 8, D->device, src, P.device, n_in * 32, st[j]));
      }
    }
    if (j > 0 && own_n[j] &&
        (rc = run_transform(dsc[j], ext, (uint32_t)n_in, (uint32_t)N, ext, (uint32_t)N, (uint32_t)N, (uint32_t)own_n[j], ext_k, (const uint32_t*)ext_omega, scales, 3,
                            nullptr, 0, st[j])) != ZKHIP_OK) return rc;
    HIPCHK(hipEventRecord(D->q_transformed, st[j]));
  }
  if ((rc = F.dev(0)) != ZKHIP_OK) return rc;
  prof_mark(s, "transform");
  // C: windows, the window kernel, the results into d_out
  std::vector<const void*> win(n_columns ? n_columns : 1);
  for (int j = 0; j < S; j++) {
    device_ctx* D = g_ctx.devs[(size_t)j];
    if ((rc = F.dev(j)) != ZKHIP_OK) return rc;
    for (int i = 0; i < S; i++)
      if (own_n[i]) HIPCHK(hipStreamWaitEvent(st[j], g_ctx.devs[(size_t)i]->q_transformed, 0));
    const size_t W = halo_lo + row_n[j] + halo_hi;
    uint32_t slot = 0;                                     // this device's window buffers, one per copied column
    for (uint32_t c = 0; c < n_columns; c++) {
      if (rs_set[c]) { win[c] = rs_window(j, c); continue; }
      const uint32_t* src;
      int src_dev;
      if (forms[c] == ZKHIP_COL_EXTENDED) { src = (const uint32_t*)d_columns[c]; src_dev = P.device; }
      else {
        const size_t ci = (size_t)(std::lower_bound(coeff_cols.begin(), coeff_cols.end(), c) - coeff_cols.begin());
        int o = 0;
        while (ci >= own_lo[o] + own_n[o]) o++;
        src = (const uint32_t*)g_ctx.devs[(size_t)o]->q_ext.p + (ci - own_lo[o]) * N * 8;
        src_dev = g_ctx.devs[(size_t)o]->device;
      }
      uint32_t* dst = (uint32_t*)D->q_win.p + (size_t)slot++ * W * 8;
      win[c] = dst;
      if ((rc = copy_window(dst, D->device, src, src_dev, window_start(row_lo[j], halo_lo, N), W, N, st[j])) != ZKHIP_OK) return rc;
    }
    if (j == 0) prof_mark(s, "exchange");
    uint32_t* out = j == 0 ? (uint32_t*)d_out + row_lo[0] * 8 : (uint32_t*)D->q_out.p;
    int compiled = 0;
    vm_call c;
    if ((rc = dsc[j]->vm_call_for(st[j], prog, 1, win.data(), n_columns, ext_k, &c)) != ZKHIP_OK) return rc;
    c.form = VM_WINDOW; c.row0 = row_lo[j]; c.count = row_n[j]; c.d_out = out; c.compiled = &compiled;
    if ((rc = row_vm_launch(c)) != ZKHIP_OK) return rc;
    if ((rc = rs_touch(j, st[j])) != ZKHIP_OK) return rc;
    if (j == 0) prof_mark(s, compiled ? "rows_compiled" : "rows_interpreted");
    else HIPCHK(hipMemcpyPeerAsync((uint32_t*)d_out + row_lo[j] * 8, P.device, out, D->device, row_n[j] * 32, st[j]));
    HIPCHK(hipEventRecord(D->q_done, st[j]));
    D->q_done_live = true;
  }
  // D: the caller's stream waits for every device (their q_done events are what F.end() would record: this call is complete without it)
  if ((rc = F.dev(0)) != ZKHIP_OK) return rc;
  for (int j = 1; j < S; j++) HIPCHK(hipStreamWaitEvent(s, g_ctx.devs[(size_t)j]->q_done, 0));
  prof_mark(s, "gather");
  F.armed = false;
  return ZKHIP_OK;
}

// ---- row-shard sets (include/zkhip.h) -------------------------------------------------------------------------------------
int zkhip_row_shards_create(uint32_t ext_k, uint32_t n_cols, uint32_t halo_lo, uint32_t halo_hi, zkhip_row_shards** out) {
  ZK_API_RANGE();
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  if (!out) { set_error("row_shards_create: null pointer"); return ZKHIP_EINVAL; }
  *out = nullptr;
  if (ext_k > 28 || n_cols == 0 || (uint64_t)halo_lo + halo_hi >= ((uint64_t)1 << 31)) {
    set_error("row_shards_create: ext_k = %u, n_cols = %u, halos %u + %u", ext_k, n_cols, halo_lo, halo_hi);
    return ZKHIP_EINVAL;
  }
  const int S = (int)g_ctx.devs.size();
  const size_t N = (size_t)1 << ext_k;
  row_shards_t* R = new row_shards_t();
  R->ext_k = ext_k; R->n_cols = n_cols; R->halo_lo = halo_lo; R->halo_hi = halo_hi; R->S = S;
  R->mem.assign((size_t)S, nullptr);
  R->last.resize((size_t)S);
  for (int j = 0; j < S; j++) {
    size_t lo, hi;
    shard_range(N, j, S, &lo, &hi);
    R->row0.push_back(lo);
    R->count.push_back(hi - lo);
  }
  for (int j = 0; j < S; j++) {
    (void)hipSetDevice(g_ctx.devs[(size_t)j]->device);
    const size_t bytes = (size_t)n_cols * R->W(j) * 32;
    if (hipMalloc(&R->mem[(size_t)j], std::max<size_t>(bytes, 32)) != hipSuccess) {
      (void)hipGetLastError();
      R->mem[(size_t)j] = nullptr;
      free_row_shards(R);
      set_error("row_shards_create: hipMalloc(%zu) failed on device %d", bytes, j);
      return ZKHIP_ENOMEM;
    }
  }
  (void)hipSetDevice(primary().device);
  const uintptr_t h = g_ctx.next_set;
  g_ctx.next_set += 0x10;
  g_ctx.sets[h] = R;
  *out = (zkhip_row_shards*)h;
  return ZKHIP_OK;
}

int zkhip_row_shards_destroy(zkhip_row_shards* set) {
  ZK_API_RANGE();
  guard_t g(g_mu);
  auto it = g_ctx.sets.find((uintptr_t)set);
  if (!set || it == g_ctx.sets.end()) { set_error("row_shards_destroy: not a live row-shard set"); return ZKHIP_EINVAL; }
  row_shards_t* R = it->second;
  g_ctx.sets.erase(it);
  free_row_shards(R);
  return ZKHIP_OK;
}

int zkhip_row_shards_window(const zkhip_row_shards* set, uint32_t shard, uint32_t col, void** d_window, int* device, uint64_t* row0, uint64_t* count) {
  ZK_API_RANGE();
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  row_shards_t* R = find_row_shards(set, "row_shards_window");
  if (!R) return ZKHIP_EINVAL;
  if (shard >= (uint32_t)R->S || col >= R->n_cols) { set_error("row_shards_window: shard %u / col %u out of range (%d shards, %u columns)", shard, col, R->S, R->n_cols); return ZKHIP_EINVAL; }
  if (d_window) *d_window = R->window((int)shard, col);
  if (device) *device = g_ctx.devs[shard]->device;
  if (row0) *row0 = R->row0[shard];
  if (count) *count = R->count[shard];
  return ZKHIP_OK;
}

int zkhip_row_shards_scatter_device(zkhip_row_shards* set, uint32_t col, const void* d_src, void* stream) {
  ZK_API_RANGE();
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  row_shards_t* R = find_row_shards(set, "row_shards_scatter");
  if (!R) return ZKHIP_EINVAL;
  if (col >= R->n_cols || !d_src) { set_error("row_shards_scatter: col %u out of range or null source", col); return ZKHIP_EINVAL; }
  const size_t N = (size_t)1 << R->ext_k;
  std::unique_lock<std::mutex> fan(g_fanout_mu);
  fan_call F;
  if ((rc = F.begin(caller_stream(stream))) != ZKHIP_OK) return rc;
  for (int j = 0; j < R->S; j++) {
    if ((rc = F.dev(j)) != ZKHIP_OK) return rc;
    if ((rc = copy_window(R->window(j, col), g_ctx.devs[(size_t)j]->device, (const uint32_t*)d_src, primary().device, window_start(R->row0[(size_t)j], R->halo_lo, N),
                          R->W(j), N, F.st[(size_t)j])) != ZKHIP_OK) return rc;
    if ((rc = touch_row_shards(R, j, F.st[(size_t)j])) != ZKHIP_OK) return rc;
  }
  return F.end();
}

int zkhip_row_shards_gather_device(const zkhip_row_shards* set, uint32_t col, void* d_dst, void* stream) {
  ZK_API_RANGE();
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  row_shards_t* R = find_row_shards(set, "row_shards_gather");
  if (!R) return ZKHIP_EINVAL;
  if (col >= R->n_cols || !d_dst) { set_error("row_shards_gather: col %u out of range or null destination", col); return ZKHIP_EINVAL; }
  std::unique_lock<std::mutex> fan(g_fanout_mu);
  fan_call F;
  if ((rc = F.begin(caller_stream(stream))) != ZKHIP_OK) return rc;
  for (int j = 0; j < R->S; j++) {
    if ((rc = F.dev(j)) != ZKHIP_OK) return rc;
    if (R->count[(size_t)j])
      HIPCHK(hipMemcpyPeerAsync((uint32_t*)d_dst + R->row0[(size_t)j] * 8, primary().device, R->window(j, col) + R->halo_lo * 8, g_ctx.devs[(size_t)j]->device,
                                R->count[(size_t)j] * 32, F.st[(size_t)j]));
    if ((rc = touch_row_shards(R, j, F.st[(size_t)j])) != ZKHIP_OK) return rc;
  }
  return F.end();
}

int zkhip_row_shards_upload(zkhip_row_shards* set, uint32_t col, const void* host_src) {
  ZK_API_RANGE();
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  row_shards_t* R = find_row_shards(set, "row_shards_upload");
  if (!R) return ZKHIP_EINVAL;
  if (col >= R->n_cols || !host_src) { set_error("row_shards_upload: col %u out of range or null source", col); return ZKHIP_EINVAL; }
  const size_t N = (size_t)1 << R->ext_k;
  wait_row_shards(R);                                      // earlier work on the set (readers included) is done before it is overwritten
  for (int j = 0; j < R->S; j++) {
    if (hipSetDevice(g_ctx.devs[(size_t)j]->device) != hipSuccess) { set_error("hipSetDevice failed"); return ZKHIP_ENODEV; }
    uint32_t* dst = R->window(j, col);
    const uint32_t* src = (const uint32_t*)host_src;
    const size_t W = R->W(j);
    for (size_t t = 0, pos = window_start(R->row0[(size_t)j], R->halo_lo, N); t < W;) {
      const size_t len = std::min(W - t, N - pos);
      if (hipMemcpy(dst + t * 8, src + pos * 8, len * 32, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError(); (void)hipSetDevice(primary().device); set_error("row_shards_upload: copy to device %d failed", j); return ZKHIP_EHIP;
      }
      t += len;
      pos = 0;
    }
  }
  (void)hipSetDevice(primary().device);
  return ZKHIP_OK;
}

int zkhip_coeff_to_extended_row_shards_device(const void* d_coeff, uint32_t k, uint32_t n_polys, size_t coeff_stride, const uint64_t ext_omega[4],
                                              const uint64_t zeta[4], zkhip_row_shards* set, uint32_t col0, void* stream) {
  ZK_API_RANGE();
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  row_shards_t* R = find_row_shards(set, "coeff_to_extended_row_shards");
  if (!R) return ZKHIP_EINVAL;
  if (!ext_omega || !zeta || (n_polys && !d_coeff)) { set_error("coeff_to_extended_row_shards: null pointer"); return ZKHIP_EINVAL; }
  if (k > R->ext_k || (uint64_t)col0 + n_polys > R->n_cols || coeff_stride < ((size_t)1 << k) || coeff_stride >= ((size_t)1 << 32)) {
    set_error("coeff_to_extended_row_shards: k = %u (ext_k %u), columns %u + %u of %u, stride %zu", k, R->ext_k, col0, n_polys, R->n_cols, coeff_stride);
    return ZKHIP_EINVAL;
  }
  if (n_polys == 0) return ZKHIP_OK;
  const uint32_t ext_k = R->ext_k;
  const size_t N = (size_t)1 << ext_k, n_in = (size_t)1 << k;
  uint32_t scales[24];
  coset_scales(zeta, nullptr, scales);
  hipStream_t s = caller_stream(stream);
  std::unique_lock<std::mutex> fan(g_fanout_mu);
  fan_call F;
  if ((rc = F.begin(s)) != ZKHIP_OK) return rc;
  for (int j = 0; j < R->S; j++) {
    size_t lo, hi;
    shard_range(n_polys, j, R->S, &lo, &hi);
    if (lo == hi) continue;
    device_ctx* D = g_ctx.devs[(size_t)j];
    if ((rc = F.dev(j)) != ZKHIP_OK) return rc;
    hipStream_t st = F.st[(size_t)j];
    scratch* dsc = scratch_for(*D, st);
    if ((rc = dsc->q_ext.reserve(N * 32)) != ZKHIP_OK) return rc;
    uint32_t* ext = (uint32_t*)dsc->q_ext.p;
    for (size_t c = lo; c < hi; c++) {
      const uint32_t* src = (const uint32_t*)d_coeff + c * coeff_stride * 8;
      if ((rc = F.dev(j)) != ZKHIP_OK) return rc;
      if (j == 0) {
        if ((rc = run_transform(dsc, src, (uint32_t)n_in, (uint32_t)n_in, ext, (uint32_t)N, (uint32_t)N, 1, ext_k, (const uint32_t*)ext_omega, scales, 3, nullptr, 0,
                                st)) != ZKHIP_OK) return rc;
      } else {
        HIPCHK(hipMemcpyPeerAsync(ext, D->device, src, primary().device, n_in * 32, st));
        if ((rc = run_transform(dsc, ext, (uint32_t)n_in, (uint32_t)N, ext, (uint32_t)N, (uint32_t)N, 1, ext_k, (const uint32_t*)ext_omega, scales, 3, nullptr, 0,
                                st)) != ZKHIP_OK) return rc;
      }
      for (int i = 0; i < R->S; i++)
        if ((rc = copy_window(R->window(i, col0 + (uint32_t)c), g_ctx.devs[(size_t)i]->device, ext, D->device, window_start(R->row0[(size_t)i], R->halo_lo, N),
                              R->W(i), N, st)) != ZKHIP_OK) return rc;
    }
    if ((rc = touch_row_shards(R, j, st)) != ZKHIP_OK) return rc;
  }
  return F.end();
}

int zkhip_lagrange_cosets_row_shards_device(uint32_t k, uint64_t usable_rows, const uint64_t omega[4], const uint64_t ext_omega[4], const uint64_t zeta[4],
                                            zkhip_row_shards* set, uint32_t col0, void* stream) {
  ZK_API_RANGE();
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  row_shards_t* R = find_row_shards(set, "lagrange_cosets_row_shards");
  if (!R) return ZKHIP_EINVAL;
  if (!omega || !ext_omega || !zeta) { set_error("lagrange_cosets_row_shards: null pointer"); return ZKHIP_EINVAL; }
  const uint64_t n = (uint64_t)1 << (k > 28 ? 0 : k);
  if (k > R->ext_k || usable_rows < 1 || usable_rows >= n || (uint64_t)col0 + 3 > R->n_cols) {
    set_error("lagrange_cosets_row_shards: k = %u (ext_k %u), u = %llu, columns %u + 3 of %u", k, R->ext_k, (unsigned long long)usable_rows, col0, R->n_cols);
    return ZKHIP_EINVAL;
  }
  namespace hd = zkhip::halo2::detail;
  typedef zkhip::halo2::Fr fr;
  const uint64_t N = (uint64_t)1 << R->ext_k, u = usable_rows;
  const bool sum_below = u <= n - u;                         // l_active over the shorter side of the active rows
  const uint64_t a0 = sum_below ? 0 : u, n_terms = sum_below ? u : n - u;
  fr z, we, w;
  memcpy(z.l, zeta, 32); memcpy(we.l, ext_omega, 32); memcpy(w.l, omega, 32);
  const fr step = hd::pow_u64(we, 64 % N), step_inv = hd::pow_u64(we, (N - 64 % N) % N);
  const fr c[10] = {z, we, step, step_inv, hd::pow_u64(step, n), hd::pow_u64(step_inv, n), hd::invert(hd::from_u64(n)), w, hd::pow_u64(w, u), hd::pow_u64(w, a0)};
  uint32_t consts[10][8];
  for (int i = 0; i < 10; i++) memcpy(consts[i], c[i].l, 32);
  std::unique_lock<std::mutex> fan(g_fanout_mu);
  fan_call F;
  if ((rc = F.begin(caller_stream(stream))) != ZKHIP_OK) return rc;
  for (int j = 0; j < R->S; j++) {
    if ((rc = F.dev(j)) != ZKHIP_OK) return rc;
    if ((rc = fr_lagrange_cosets_window_device(R->window(j, col0), R->window(j, col0 + 1), R->window(j, col0 + 2), R->W(j), window_start(R->row0[(size_t)j], R->halo_lo, N),
                                               k, R->ext_k, (uint32_t)n_terms, sum_below ? 1 : 0, consts, F.st[(size_t)j])) != ZKHIP_OK) return rc;
    if ((rc = touch_row_shards(R, j, F.st[(size_t)j])) != ZKHIP_OK) return rc;
  }
  return F.end();
}

// The straight-line HIP source rowvm_jit.hip generates for `prog` (buf may be NULL: *len receives the size needed, NUL included), and a
// compile-only run of it through hiprtc -- no device needed (the generator's CPU-side test; a host may also use it to warm hiprtc's caches at keygen).
int zkhip_vm_jit_source(const zkhip_vm_program* prog, uint32_t n_columns, uint32_t log_rows, char* buf, size_t cap, size_t* len) {
  ZK_API_RANGE();
  int rc = row_vm_validate(prog, n_columns, log_rows, 0);
  if (rc != ZKHIP_OK) return rc;
  std::string src;
  if ((rc = row_vm_jit_source(prog, n_columns, log_rows, &src)) != ZKHIP_OK) return rc;
  if (len) *len = src.size() + 1;
  if (buf && cap) { const size_t m = std::min(cap - 1, src.size()); memcpy(buf, src.data(), m); buf[m] = 0; }
  return ZKHIP_OK;
}

int zkhip_vm_jit_compile(const zkhip_vm_program* prog, uint32_t n_columns, uint32_t log_rows, size_t* code_bytes) {
  ZK_API_RANGE();
  int rc = row_vm_validate(prog, n_columns, log_rows, 0);
  if (rc != ZKHIP_OK) return rc;
  return row_vm_jit_compile_only(prog, n_columns, log_rows, code_bytes);
}

// Which executor ran: the interpreter takes every call the compiled one does not (hiprtc missing, a failed compilation, a program outside
// the limits) with the same results, so a test that compares the two reads this before and after a call.
uint64_t zkhip_test_rows_compiled_count(void) { return row_vm_jit_launches(); }

int zkhip_fr_eval_rows(const zkhip_vm_program* prog, const uint64_t* const* columns, uint32_t n_columns, uint32_t log_rows,
                       int accumulate, uint64_t* out) {
  ZK_API_RANGE();
  int rc;
  if ((rc = row_vm_validate(prog, n_columns, log_rows, accumulate)) != ZKHIP_OK) return rc;
  if (!out || (n_columns && !columns)) { set_error("eval_rows: null pointer"); return ZKHIP_EINVAL; }
  for (uint32_t i = 0; i < n_columns; i++)
    if (!columns[i]) { set_error("eval_rows: column %u is null", i); return ZKHIP_EINVAL; }
  lane_hold H;
  if (H.rc != ZKHIP_OK) return H.rc;
  const size_t rows = (size_t)1 << log_rows, bytes = rows * 32;
  hipStream_t s = H.s;
  if ((rc = H.sc->poly.reserve((size_t)(n_columns ? n_columns : 1) * bytes)) != ZKHIP_OK) return rc;
  if ((rc = H.sc->poly2.reserve(bytes)) != ZKHIP_OK) return rc;
  std::vector<const void*> d_cols(n_columns);
  for (uint32_t i = 0; i < n_columns; i++) {
    d_cols[i] = (char*)H.sc->poly.p + (size_t)i * bytes;
    HIPCHK(hipMemcpyAsync((void*)d_cols[i], columns[i], bytes, hipMemcpyHostToDevice, s));
  }
  if (accumulate) HIPCHK(hipMemcpyAsync(H.sc->poly2.p, out, bytes, hipMemcpyHostToDevice, s));
  if ((rc = zkhip_fr_eval_rows_device(prog, d_cols.data(), n_columns, log_rows, accumulate, H.sc->poly2.p, s)) != ZKHIP_OK) return rc;
  HIPCHK(hipMemcpyAsync(out, H.sc->poly2.p, bytes, hipMemcpyDeviceToHost, s));
  return H.finish();
}

int zkhip_fr_gather_mul_device(const void* d_a, size_t a_len, const void* d_index_a, const void* d_b, size_t b_len, const void* d_index_b, size_t n,
                               void* d_out, void* stream) {
  ZK_API_RANGE();
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  if (n && (!d_a || !d_b || !d_index_a || !d_index_b || !d_out || a_len == 0 || b_len == 0 || a_len >= ((size_t)1 << 32) || b_len >= ((size_t)1 << 32))) {
    set_error("gather_mul: bad argument");
    return ZKHIP_EINVAL;
  }
  return fr_gather_mul_device((const uint32_t*)d_a, (uint32_t)a_len, (const uint32_t*)d_index_a, (const uint32_t*)d_b, (uint32_t)b_len, (const uint32_t*)d_index_b, n,
                              (uint32_t*)d_out, caller_stream(stream));
}

int zkhip_fr_grand_product_device(const void* d_num, void* d_den, size_t n, void* d_z, void* stream) {
  ZK_API_RANGE();
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  if (n && (!d_num || !d_den || !d_z)) { set_error("grand_product: null pointer"); return ZKHIP_EINVAL; }
  if (n == 0) return ZKHIP_OK;
  hipStream_t s = caller_stream(stream);
  if ((rc = zkhip_fr_batch_invert_device(d_den, n, s)) != ZKHIP_OK) return rc;
  if ((rc = fr_pointwise_mul_device((const uint32_t*)d_num, (const uint32_t*)d_den, n, (uint32_t*)d_den, s)) != ZKHIP_OK) return rc;
  return zkhip_fr_prefix_product_device(d_den, n, d_z, s);
}

int zkhip_fr_grand_product(const uint64_t* num, const uint64_t* den, size_t n, uint64_t* z) {
  ZK_API_RANGE();
  if (n && (!num || !den || !z)) { set_error("grand_product: null pointer"); return ZKHIP_EINVAL; }
  if (n == 0) return ZKHIP_OK;
  lane_hold H;
  if (H.rc != ZKHIP_OK) return H.rc;
  int rc;
  hipStream_t s = H.s;
  if ((rc = H.sc->poly.reserve(n * 32)) != ZKHIP_OK) return rc;
  if ((rc = H.sc->poly2.reserve(n * 32)) != ZKHIP_OK) return rc;
  HIPCHK(hipMemcpyAsync(H.sc->poly.p, num, n * 32, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(H.sc->poly2.p, den, n * 32, hipMemcpyHostToDevice, s));
  if ((rc = zkhip_fr_grand_product_device(H.sc->poly.p, H.sc->poly2.p, n, H.sc->poly.p, s)) != ZKHIP_OK) return rc;
  HIPCHK(hipMemcpyAsync(z, H.sc->poly.p, n * 32, hipMemcpyDeviceToHost, s));
  return H.finish();
}

int zkhip_fr_linear_combination_device(const void* const* d_cols, const uint64_t* coeffs, size_t count, size_t n, void* d_out, void* stream) {
  ZK_API_RANGE();
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  if (n && (!d_out || (count && (!d_cols || !coeffs)))) { set_error("linear_combination: null pointer"); return ZKHIP_EINVAL; }
  for (size_t i = 0; i < count && n; i++)
    if (!d_cols[i]) { set_error("linear_combination: column %zu is null", i); return ZKHIP_EINVAL; }
  if (n == 0) return ZKHIP_OK;
  hipStream_t s = caller_stream(stream);
  scratch* sc = scratch_for(primary(), s);
  if ((rc = sc->ws.reserve(lincomb_workspace_bytes(count, n))) != ZKHIP_OK) return rc;
  return fr_linear_combination_device(d_cols, (const uint32_t*)coeffs, count, n, (uint32_t*)d_out, sc->ws.p, sc->ws.cap, s, &sc->args);
}

static int perm_args_ok(const void* const* values, const void* const* sigmas, uint32_t n_columns, uint32_t chunk_len, uint32_t log_n, size_t usable_rows,
                        const uint64_t* beta, const uint64_t* gamma, const uint64_t* delta, const uint64_t* omega, const void* z) {
  if (n_columns == 0) return ZKHIP_OK;
  if (!values || !sigmas || !beta || !gamma || !delta || !omega || !z) { set_error("permutation_products: null pointer"); return ZKHIP_EINVAL; }
  if (chunk_len == 0 || log_n > 28 || usable_rows > ((size_t)1 << log_n)) {
    set_error("permutation_products: bad shape (chunk_len %u, log_n %u, usable_rows %zu)", chunk_len, log_n, usable_rows);
    return ZKHIP_EINVAL;
  }
  for (uint32_t i = 0; i < n_columns; i++)
    if (!values[i] || !sigmas[i]) { set_error("permutation_products: column %u is null", i); return ZKHIP_EINVAL; }
  return ZKHIP_OK;
}

int zkhip_permutation_products_device(const void* const* d_values, const void* const* d_sigmas, uint32_t n_columns, uint32_t chunk_len, uint32_t log_n,
                                      size_t usable_rows, const uint64_t beta[4], const uint64_t gamma[4], const uint64_t delta[4], const uint64_t omega[4],
                                      void* d_z, void* stream) {
  ZK_API_RANGE();
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  if ((rc = perm_args_ok(d_values, d_sigmas, n_columns, chunk_len, log_n, usable_rows, beta, gamma, delta, omega, d_z)) != ZKHIP_OK) return rc;
  if (n_columns == 0) return ZKHIP_OK;
  hipStream_t s = caller_stream(stream);
  scratch* sc = scratch_for(primary(), s);
  if ((rc = sc->ws.reserve(perm_workspace_bytes(n_columns, chunk_len, log_n))) != ZKHIP_OK) return rc;
  return fr_permutation_products_device(d_values, d_sigmas, n_columns, chunk_len, log_n, usable_rows, (const uint32_t*)beta, (const uint32_t*)gamma,
                                        (const uint32_t*)delta, (const uint32_t*)omega, (uint32_t*)d_z, sc->ws.p, sc->ws.cap, s, &sc->args);
}

int zkhip_permutation_products(const uint64_t* const* values, const uint64_t* const* sigmas, uint32_t n_columns, uint32_t chunk_len, uint32_t log_n,
                               size_t usable_rows, const uint64_t beta[4], const uint64_t gamma[4], const uint64_t delta[4], const uint64_t omega[4],
                               uint64_t* z) {
  ZK_API_RANGE();
  int rc;
  if ((rc = perm_args_ok((const void* const*)values, (const void* const*)sigmas, n_columns, chunk_len, log_n, usable_rows, beta, gamma, delta, omega, z)) != ZKHIP_OK)
    return rc;
  if (n_columns == 0) return ZKHIP_OK;
  lane_hold H;
  if (H.rc != ZKHIP_OK) return H.rc;
  hipStream_t s = H.s;
  const size_t n = (size_t)1 << log_n, bytes = n * 32, nsets = (n_columns + chunk_len - 1) / chunk_len;
  if ((rc = H.sc->poly.reserve((size_t)2 * n_columns * bytes)) != ZKHIP_OK) return rc;
  if ((rc = H.sc->poly2.reserve(nsets * bytes)) != ZKHIP_OK) return rc;
  std::vector<const void*> d_cols((size_t)2 * n_columns);
  for (uint32_t i = 0; i < n_columns; i++) {
    d_cols[i] = (char*)H.sc->poly.p + (size_t)i * bytes;
    d_cols[n_columns + i] = (char*)H.sc->poly.p + (size_t)(n_columns + i) * bytes;
    HIPCHK(hipMemcpyAsync((void*)d_cols[i], values[i], bytes, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync((void*)d_cols[n_columns + i], sigmas[i], bytes, hipMemcpyHostToDevice, s));
  }
  if ((rc = zkhip_permutation_products_device(d_cols.data(), d_cols.data() + n_columns, n_columns, chunk_len, log_n, usable_rows, beta, gamma, delta, omega,
                                              H.sc->poly2.p, s)) != ZKHIP_OK) return rc;
  HIPCHK(hipMemcpyAsync(z, H.sc->poly2.p, nsets * bytes, hipMemcpyDeviceToHost, s));
  return H.finish();
}

int zkhip_profile_enable(int on) {
  guard_t g(g_mu);
  g_prof_mode = on == 2 ? 2 : (on != 0 ? 1 : 0);
  g_prof_n = 0;
  g_prof_base = 0;
  g_prof_ncalls = 0;
  g_prof_full = false;
  return ZKHIP_OK;
}

int zkhip_profile_read(double* ms, char (*names)[64], int max) {
  ZK_API_RANGE();
  guard_t g(g_mu);
  if (!g_prof_ev_ready || g_prof_n == 0 || g_prof_mode == 2) return 0;
  if (hipEventSynchronize(g_prof_ev[g_prof_n]) != hipSuccess) { set_error("profile_read: event sync failed"); return ZKHIP_EHIP; }
  for (int i = 0; i < g_prof_n && i < max; i++) {
    float t = 0;
    (void)hipEventElapsedTime(&t, g_prof_ev[i], g_prof_ev[i + 1]);
    if (ms) ms[i] = t;
    if (names) snprintf(names[i], 64, "%s", g_prof_names[i]);
  }
  return g_prof_n;
}

int zkhip_profile_read_calls(double* ms, char (*names)[64], int* call_of, int max) {
  ZK_API_RANGE();
  guard_t g(g_mu);
  if (!g_prof_ev_ready || g_prof_mode != 2 || g_prof_ncalls == 0) return 0;
  if (!g_prof_full) g_prof_calls[g_prof_ncalls - 1][1] = g_prof_n;
  int out = 0;
  for (int c = 0; c < g_prof_ncalls; c++) {
    const int base = g_prof_calls[c][0], n = g_prof_calls[c][1];
    if (n == 0) continue;
    if (hipEventSynchronize(g_prof_ev[base + n]) != hipSuccess) { set_error("profile_read_calls: event sync failed"); return ZKHIP_EHIP; }
    for (int i = 0; i < n && out < max; i++, out++) {
      float t = 0;
      (void)hipEventElapsedTime(&t, g_prof_ev[base + i], g_prof_ev[base + i + 1]);
      if (ms) ms[out] = t;
      if (names) snprintf(names[out], 64, "%s", g_prof_names[base + i]);
      if (call_of) call_of[out] = c;
    }
  }
  return out;
}

int zkhip_g1_fixed_base_mul_device(const void* d_scalars, size_t n, void* d_out, void* stream) {
  ZK_API_RANGE();
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  if (n && (!d_scalars || !d_out)) { set_error("fixed_base_mul: null pointer"); return ZKHIP_EINVAL; }
  if (n == 0) return ZKHIP_OK;
  hipStream_t s = caller_stream(stream);
  scratch* sc = scratch_for(primary(), s);
  device_ctx& P = primary();
  if ((rc = sc->ws.reserve(g1_fixed_base_workspace(n))) != ZKHIP_OK) return rc;
  if (!P.fixed_table_ready) {              // one-time: 16 windows x 2^15 multiples of the generator (32 MiB), shared by every stream
    if ((rc = P.fixed_table.reserve(g1_fixed_base_table_bytes())) != ZKHIP_OK) return rc;
    if ((rc = g1_fixed_base_table_build((uint32_t*)P.fixed_table.p, sc->ws.p, sc->ws.cap, s)) != ZKHIP_OK) return rc;
    HIPCHK(hipStreamSynchronize(s));
    P.fixed_table_ready = true;
  }
  return g1_fixed_base_mul_device((const uint32_t*)d_scalars, n, (const uint32_t*)P.fixed_table.p, (uint32_t*)d_out, sc->ws.p, sc->ws.cap, s);
}

int zkhip_g1_fft_device(void* d_points_xyz, const uint64_t omega[4], uint32_t log_n, void* stream) {
  ZK_API_RANGE();
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  if (!d_points_xyz || !omega) { set_error("g1_fft: null pointer"); return ZKHIP_EINVAL; }
  if (log_n > 26) { set_error("g1_fft: log_n = %u out of range", log_n); return ZKHIP_EINVAL; }
  const size_t n = (size_t)1 << log_n;
  hipStream_t s = caller_stream(stream);
  scratch* sc = scratch_for(primary(), s);
  if ((rc = sc->ws.reserve(g1_fft_workspace(n))) != ZKHIP_OK) return rc;
  return g1_fft_device((const uint32_t*)d_points_xyz, 1, (uint32_t*)d_points_xyz, 1, log_n, (const uint32_t*)omega, nullptr, sc->ws.p, sc->ws.cap, s);
}

int zkhip_g_to_lagrange_device(const void* d_g, uint32_t k, void* d_g_lagrange, void* stream) {
  ZK_API_RANGE();
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  if (!d_g || !d_g_lagrange) { set_error("g_to_lagrange: null pointer"); return ZKHIP_EINVAL; }
  if (d_g == d_g_lagrange) { set_error("g_to_lagrange: the arrays may not alias"); return ZKHIP_EINVAL; }
  if (k > 26) { set_error("g_to_lagrange: k = %u out of range", k); return ZKHIP_EINVAL; }
  const size_t n = (size_t)1 << k;
  hipStream_t s = caller_stream(stream);
  scratch* sc = scratch_for(primary(), s);
  if ((rc = sc->ws.reserve(g1_fft_workspace(n))) != ZKHIP_OK) return rc;
  namespace H = zkhip::halo2;
  H::Fr omega = H::fr_root_of_unity();
  for (uint32_t i = k; i < 28; i++) omega = H::detail::mul(omega, omega);
  const H::Fr omega_inv = H::detail::invert(omega), n_inv = H::detail::invert(H::detail::from_u64((uint64_t)n));
  return g1_fft_device((const uint32_t*)d_g, 0, (uint32_t*)d_g_lagrange, 0, k, (const uint32_t*)omega_inv.l, (const uint32_t*)n_inv.l, sc->ws.p, sc->ws.cap, s);
}

// host-buffer form, with the memory of the reference's `g_to_lagrange(g_projective: Vec<C::Curve>, k) -> Vec<C>`: 2^k Jacobian points in, 2^k affine
// points out (the whole function: inverse FFT over the points, the 1/n scaling and Curve::batch_normalize in one call)
int zkhip_g_to_lagrange(const uint64_t* g_xyz, uint32_t k, uint64_t* g_lagrange) {
  ZK_API_RANGE();
  if (!g_xyz || !g_lagrange) { set_error("g_to_lagrange: null pointer"); return ZKHIP_EINVAL; }
  if (k > 26) { set_error("g_to_lagrange: k = %u out of range", k); return ZKHIP_EINVAL; }
  lane_hold H;
  if (H.rc != ZKHIP_OK) return H.rc;
  int rc;
  const size_t n = (size_t)1 << k;
  hipStream_t s = H.s;
  scratch* sc = H.sc;
  if ((rc = sc->bases.reserve(n * 96)) != ZKHIP_OK) return rc;
  if ((rc = sc->poly.reserve(n * 64)) != ZKHIP_OK) return rc;
  if ((rc = sc->ws.reserve(g1_fft_workspace(n))) != ZKHIP_OK) return rc;
  HIPCHK(hipMemcpyAsync(sc->bases.p, g_xyz, n * 96, hipMemcpyHostToDevice, s));
  namespace Hh = zkhip::halo2;
  Hh::Fr omega = Hh::fr_root_of_unity();
  for (uint32_t i = k; i < 28; i++) omega = Hh::detail::mul(omega, omega);
  const Hh::Fr omega_inv = Hh::detail::invert(omega), n_inv = Hh::detail::invert(Hh::detail::from_u64((uint64_t)n));
  if ((rc = g1_fft_device((const uint32_t*)sc->bases.p, 1, (uint32_t*)sc->poly.p, 0, k, (const uint32_t*)omega_inv.l, (const uint32_t*)n_inv.l, sc->ws.p, sc->ws.cap, s)) != ZKHIP_OK) return rc;
  HIPCHK(hipMemcpyAsync(g_lagrange, sc->poly.p, n * 64, hipMemcpyDeviceToHost, s));
  return H.finish();
}

int zkhip_g1_gen_walk_device(const uint64_t t0[4], const uint64_t d[4], size_t n, void* d_out, void* stream) {
  ZK_API_RANGE();
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  if (!t0 || !d || (n && !d_out)) { set_error("gen_walk: null pointer"); return ZKHIP_EINVAL; }
  hipStream_t s = caller_stream(stream);
  scratch* sc = scratch_for(primary(), s);
  if ((rc = sc->ws.reserve(g1_gen_walk_workspace(n))) != ZKHIP_OK) return rc;
  return g1_gen_walk_device((const uint32_t*)t0, (const uint32_t*)d, n, (uint32_t*)d_out, sc->ws.p, sc->ws.cap, s);
}

// ---- Curve::batch_normalize: Jacobian commitments -> affine (what create_proof writes into the transcript) ------------------------
int zkhip_g1_batch_normalize_device(const void* d_points_xyz, size_t n, void* d_out_affine, void* stream) {
  ZK_API_RANGE();
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  if (n && (!d_points_xyz || !d_out_affine)) { set_error("batch_normalize: null pointer"); return ZKHIP_EINVAL; }
  if (n == 0) return ZKHIP_OK;
  hipStream_t s = caller_stream(stream);
  scratch* sc = scratch_for(primary(), s);
  if ((rc = sc->ws.reserve(g1_batch_normalize_workspace(n))) != ZKHIP_OK) return rc;
  return g1_batch_normalize_device((const uint32_t*)d_points_xyz, n, (uint32_t*)d_out_affine, sc->ws.p, sc->ws.cap, s);
}

int zkhip_g1_batch_normalize(const uint64_t* points_xyz, size_t n, uint64_t* out_affine) {
  ZK_API_RANGE();
  if (n && (!points_xyz || !out_affine)) { set_error("batch_normalize: null pointer"); return ZKHIP_EINVAL; }
  if (n == 0) return ZKHIP_OK;
  lane_hold H;
  if (H.rc != ZKHIP_OK) return H.rc;
  int rc;
  hipStream_t s = H.s;
  if ((rc = H.sc->poly.reserve(n * (96 + 64))) != ZKHIP_OK) return rc;
  if ((rc = H.sc->ws.reserve(g1_batch_normalize_workspace(n))) != ZKHIP_OK) return rc;
  char* d = (char*)H.sc->poly.p;
  HIPCHK(hipMemcpyAsync(d, points_xyz, n * 96, hipMemcpyHostToDevice, s));
  if ((rc = g1_batch_normalize_device((const uint32_t*)d, n, (uint32_t*)(d + n * 96), H.sc->ws.p, H.sc->ws.cap, s)) != ZKHIP_OK) return rc;
  HIPCHK(hipMemcpyAsync(out_affine, d + n * 96, n * 64, hipMemcpyDeviceToHost, s));
  return H.finish();
}

// ---- G2 MSM: best_multiexp::<G2Affine> -------------------------------------------------------------------------------
int zkhip_msm_g2_device(const void* d_scalars, const void* d_bases, size_t n, void* d_out_xyz, void* stream) {
  ZK_API_RANGE();
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  if (!d_out_xyz || (n && (!d_scalars || !d_bases))) { set_error("msm_g2: null pointer"); return ZKHIP_EINVAL; }
  hipStream_t s = caller_stream(stream);
  scratch* sc = scratch_for(primary(), s);
  if ((rc = sc->ws.reserve(msm_g2_workspace_bytes(n))) != ZKHIP_OK) return rc;
  return msm_g2_device((const uint32_t*)d_scalars, (const uint32_t*)d_bases, n, (uint32_t*)d_out_xyz, sc->ws.p, sc->ws.cap, s);
}

int zkhip_msm_g2(const uint64_t* scalars, const uint64_t* bases, size_t n, uint64_t out_xyz[24]) {
  ZK_API_RANGE();
  if (!out_xyz || (n && (!scalars || !bases))) { set_error("msm_g2: null pointer"); return ZKHIP_EINVAL; }
  lane_hold H;
  if (H.rc != ZKHIP_OK) return H.rc;
  int rc;
  hipStream_t s = H.s;
  if ((rc = H.sc->small.reserve(4096)) != ZKHIP_OK) return rc;
  if (n) {
    if ((rc = H.sc->scalars.reserve(n * 32)) != ZKHIP_OK) return rc;
    if ((rc = H.sc->bases.reserve(n * 128)) != ZKHIP_OK) return rc;
    if ((rc = H.sc->ws.reserve(msm_g2_workspace_bytes(n))) != ZKHIP_OK) return rc;
    HIPCHK(hipMemcpyAsync(H.sc->scalars.p, scalars, n * 32, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(H.sc->bases.p, bases, n * 128, hipMemcpyHostToDevice, s));
  }
  if ((rc = msm_g2_device((const uint32_t*)H.sc->scalars.p, (const uint32_t*)H.sc->bases.p, n, (uint32_t*)H.sc->small.p, H.sc->ws.p, H.sc->ws.cap, s)) != ZKHIP_OK) return rc;
  HIPCHK(hipMemcpyAsync(H.L->pinned, H.sc->small.p, 192, hipMemcpyDeviceToHost, s));
  if ((rc = H.finish()) != ZKHIP_OK) return rc;
  memcpy(out_xyz, H.L->pinned, 192);
  return ZKHIP_OK;
}

// ---- SRS / key-file validation: every point canonical and on the curve (RawBytes readers) ------------------------------
int zkhip_g1_check_points_device(const void* d_points, size_t n, uint64_t* first_bad, void* stream) {
  ZK_API_RANGE();
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  if (!first_bad || (n && !d_points)) { set_error("g1_check_points: null pointer"); return ZKHIP_EINVAL; }
  hipStream_t s = caller_stream(stream);
  scratch* sc = scratch_for(primary(), s);
  if ((rc = sc->small.reserve(4096)) != ZKHIP_OK) return rc;
  if ((rc = g1_check_points_device((const uint32_t*)d_points, n, (unsigned long long*)sc->small.p, s)) != ZKHIP_OK) return rc;
  unsigned long long v = 0;
  HIPCHK(hipMemcpyAsync(&v, sc->small.p, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  *first_bad = (uint64_t)v;
  return ZKHIP_OK;
}

int zkhip_g1_check_points(const uint64_t* points, size_t n, uint64_t* first_bad) {
  ZK_API_RANGE();
  if (!first_bad || (n && !points)) { set_error("g1_check_points: null pointer"); return ZKHIP_EINVAL; }
  lane_hold H;
  if (H.rc != ZKHIP_OK) return H.rc;
  int rc;
  *first_bad = n;
  const size_t chunk = (size_t)1 << 24;                  // 1 GiB of points per upload
  if ((rc = H.sc->bases.reserve(std::min(n, chunk) * 64)) != ZKHIP_OK) return rc;
  if ((rc = H.sc->small.reserve(4096)) != ZKHIP_OK) return rc;
  for (size_t lo = 0; lo < n; lo += chunk) {
    const size_t m = std::min(chunk, n - lo);
    H.reopen();
    HIPCHK(hipMemcpyAsync(H.sc->bases.p, points + lo * 8, m * 64, hipMemcpyHostToDevice, H.s));
    if ((rc = g1_check_points_device((const uint32_t*)H.sc->bases.p, m, (unsigned long long*)H.sc->small.p, H.s)) != ZKHIP_OK) return rc;
    HIPCHK(hipMemcpyAsync(H.L->pinned, H.sc->small.p, 8, hipMemcpyDeviceToHost, H.s));
    if ((rc = H.finish()) != ZKHIP_OK) return rc;
    const unsigned long long v = *(const unsigned long long*)H.L->pinned;
    if (v < m) { *first_bad = lo + (size_t)v; return ZKHIP_OK; }
  }
  return ZKHIP_OK;
}

// ---- SerdeFormat::Processed: compressed G1 points (serde.hip) -------------------------------------------------------------
int zkhip_g1_compress_device(const void* d_points, size_t n, void* d_out32, int flag_layout, void* stream) {
  ZK_API_RANGE();
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  if ((n && (!d_points || !d_out32)) || flag_layout < 0 || flag_layout > 1) { set_error("g1_compress: bad argument"); return ZKHIP_EINVAL; }
  return g1_compress_device((const uint32_t*)d_points, n, (uint32_t*)d_out32, flag_layout, caller_stream(stream));
}

int zkhip_g1_decompress_device(const void* d_in32, size_t n, void* d_points, int flag_layout, uint64_t* first_bad, void* stream) {
  ZK_API_RANGE();
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  if (!first_bad || (n && (!d_in32 || !d_points)) || flag_layout < 0 || flag_layout > 1) { set_error("g1_decompress: bad argument"); return ZKHIP_EINVAL; }
  hipStream_t s = caller_stream(stream);
  scratch* sc = scratch_for(primary(), s);
  if ((rc = sc->small.reserve(4096)) != ZKHIP_OK) return rc;
  unsigned long long v = (unsigned long long)n;
  HIPCHK(hipMemcpyAsync(sc->small.p, &v, 8, hipMemcpyHostToDevice, s));
  HIPCHK(hipStreamSynchronize(s));                     // `v` is a stack variable
  if ((rc = g1_decompress_device((const uint32_t*)d_in32, n, (uint32_t*)d_points, flag_layout, (unsigned long long*)sc->small.p, s)) != ZKHIP_OK) return rc;
  HIPCHK(hipMemcpyAsync(&v, sc->small.p, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  *first_bad = (uint64_t)v;
  return ZKHIP_OK;
}

int zkhip_g1_compress(const uint64_t* points, size_t n, uint8_t* out32, int flag_layout) {
  ZK_API_RANGE();
  if ((n && (!points || !out32)) || flag_layout < 0 || flag_layout > 1) { set_error("g1_compress: bad argument"); return ZKHIP_EINVAL; }
  if (n == 0) return ZKHIP_OK;
  lane_hold H;
  if (H.rc != ZKHIP_OK) return H.rc;
  int rc;
  const size_t chunk = (size_t)1 << 23;                // 512 MiB of points per upload
  if ((rc = H.sc->bases.reserve(std::min(n, chunk) * 64)) != ZKHIP_OK) return rc;
  if ((rc = H.sc->poly.reserve(std::min(n, chunk) * 32)) != ZKHIP_OK) return rc;
  for (size_t lo = 0; lo < n; lo += chunk) {
    const size_t m = std::min(chunk, n - lo);
    H.reopen();
    HIPCHK(hipMemcpyAsync(H.sc->bases.p, points + lo * 8, m * 64, hipMemcpyHostToDevice, H.s));
    if ((rc = g1_compress_device((const uint32_t*)H.sc->bases.p, m, (uint32_t*)H.sc->poly.p, flag_layout, H.s)) != ZKHIP_OK) return rc;
    HIPCHK(hipMemcpyAsync(out32 + lo * 32, H.sc->poly.p, m * 32, hipMemcpyDeviceToHost, H.s));
    if ((rc = H.finish()) != ZKHIP_OK) return rc;
  }
  return ZKHIP_OK;
}

int zkhip_g1_decompress(const uint8_t* in32, size_t n, uint64_t* points, int flag_layout, uint64_t* first_bad) {
  ZK_API_RANGE();
  if (!first_bad || (n && (!in32 || !points)) || flag_layout < 0 || flag_layout > 1) { set_error("g1_decompress: bad argument"); return ZKHIP_EINVAL; }
  *first_bad = n;
  if (n == 0) return ZKHIP_OK;
  lane_hold H;
  if (H.rc != ZKHIP_OK) return H.rc;
  int rc;
  const size_t chunk = (size_t)1 << 23;
  if ((rc = H.sc->bases.reserve(std::min(n, chunk) * 64)) != ZKHIP_OK) return rc;
  if ((rc = H.sc->poly.reserve(std::min(n, chunk) * 32)) != ZKHIP_OK) return rc;
  if ((rc = H.sc->small.reserve(4096)) != ZKHIP_OK) return rc;
  for (size_t lo = 0; lo < n; lo += chunk) {
    const size_t m = std::min(chunk, n - lo);
    H.reopen();
    *(unsigned long long*)H.L->pinned = (unsigned long long)m;
    HIPCHK(hipMemcpyAsync(H.sc->small.p, H.L->pinned, 8, hipMemcpyHostToDevice, H.s));
    HIPCHK(hipMemcpyAsync(H.sc->poly.p, in32 + lo * 32, m * 32, hipMemcpyHostToDevice, H.s));
    if ((rc = g1_decompress_device((const uint32_t*)H.sc->poly.p, m, (uint32_t*)H.sc->bases.p, flag_layout, (unsigned long long*)H.sc->small.p, H.s)) != ZKHIP_OK) return rc;
    HIPCHK(hipMemcpyAsync(points + lo * 8, H.sc->bases.p, m * 64, hipMemcpyDeviceToHost, H.s));
    HIPCHK(hipMemcpyAsync(H.L->pinned, H.sc->small.p, 8, hipMemcpyDeviceToHost, H.s));
    if ((rc = H.finish()) != ZKHIP_OK) return rc;
    const unsigned long long v = *(const unsigned long long*)H.L->pinned;
    if (v < m) { *first_bad = lo + (size_t)v; return ZKHIP_OK; }
  }
  return ZKHIP_OK;
}

// ---- parity hooks ----------------------------------------------------------------------------------
int zkhip_test_field_op(int field, int op, const uint64_t* a, const uint64_t* b, uint64_t* out, size_t n) {
  ZK_API_RANGE();
  const bool field_op_ok = (op >= 0 && op <= 7) || (op >= 256 + 4 && op <= 256 + 7);
  if (field < 0 || field > 1 || !field_op_ok || (n && (!a || !b || !out))) { set_error("test_field_op: bad argument"); return ZKHIP_EINVAL; }
  if ((op & 255) >= 6 && (n & 1)) { set_error("test_field_op: ops 6 and 7 pair element i with i ^ 1: n must be even"); return ZKHIP_EINVAL; }
  if (n == 0) return ZKHIP_OK;
  lane_hold H;
  if (H.rc != ZKHIP_OK) return H.rc;
  int rc;
  hipStream_t s = H.s;
  if ((rc = H.sc->poly.reserve(n * 96)) != ZKHIP_OK) return rc;
  char* d = (char*)H.sc->poly.p;
  HIPCHK(hipMemcpyAsync(d, a, n * 32, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(d + n * 32, b, n * 32, hipMemcpyHostToDevice, s));
  if ((rc = test_field_op(field, op, (uint32_t*)d, (uint32_t*)(d + n * 32), (uint32_t*)(d + n * 64), n, s)) != ZKHIP_OK) return rc;
  HIPCHK(hipMemcpyAsync(out, d + n * 64, n * 32, hipMemcpyDeviceToHost, s));
  return H.finish();
}

int zkhip_test_g1_op(int op, const uint64_t* a, const uint64_t* b, uint64_t* out_xyz, size_t n) {
  ZK_API_RANGE();
  if (!((op >= 0 && op <= 6) || op == 256 + 5 || op == 256 + 6) || (n && (!a || !b || !out_xyz))) { set_error("test_g1_op: bad argument"); return ZKHIP_EINVAL; }
  if (n == 0) return ZKHIP_OK;
  lane_hold H;
  if (H.rc != ZKHIP_OK) return H.rc;
  int rc;
  hipStream_t s = H.s;
  if ((rc = H.sc->poly.reserve(n * (64 + 64 + 96))) != ZKHIP_OK) return rc;
  char* d = (char*)H.sc->poly.p;
  HIPCHK(hipMemcpyAsync(d, a, n * 64, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(d + n * 64, b, n * 64, hipMemcpyHostToDevice, s));
  if ((rc = test_g1_op(op, (uint32_t*)d, (uint32_t*)(d + n * 64), (uint32_t*)(d + n * 128), n, s)) != ZKHIP_OK) return rc;
  HIPCHK(hipMemcpyAsync(out_xyz, d + n * 128, n * 96, hipMemcpyDeviceToHost, s));
  return H.finish();
}

int zkhip_test_g2_op(int op, const uint64_t* a, const uint64_t* b, uint64_t* out_xyz, size_t n) {
  ZK_API_RANGE();
  if (!((op >= 0 && op <= 11) || (op >= 256 + 5 && op <= 256 + 11)) || (n && (!a || !b || !out_xyz))) { set_error("test_g2_op: bad argument"); return ZKHIP_EINVAL; }
  if (n == 0) return ZKHIP_OK;
  lane_hold H;
  if (H.rc != ZKHIP_OK) return H.rc;
  int rc;
  hipStream_t s = H.s;
  const bool formula_op = op >= 7;                                   // selftest.hip; op 10 keeps its two operands as work points (2 x 288 bytes a row)
  if ((rc = H.sc->poly.reserve(n * (128 + 128 + 192 + ((op & 255) == 10 ? 2 * 288 : 0)))) != ZKHIP_OK) return rc;
  char* d = (char*)H.sc->poly.p;
  HIPCHK(hipMemcpyAsync(d, a, n * 128, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(d + n * 128, b, n * 128, hipMemcpyHostToDevice, s));
  if (formula_op) rc = test_g2_formula_op(op, (uint32_t*)d, (uint32_t*)(d + n * 128), (uint32_t*)(d + n * 256), (uint32_t*)(d + n * 448), n, s);
  else rc = test_g2_op(op, (uint32_t*)d, (uint32_t*)(d + n * 128), (uint32_t*)(d + n * 256), n, s);
  if (rc != ZKHIP_OK) return rc;
  HIPCHK(hipMemcpyAsync(out_xyz, d + n * 256, n * 192, hipMemcpyDeviceToHost, s));
  return H.finish();
}

// ---- pairing check (pairing.hip) ------------------------------------------------------------------------------------------------------
int zkhip_pairing_check_device(const void* d_g1, const void* d_g2, size_t n, void* d_ok, void* stream) {
  ZK_API_RANGE();
  if (!d_ok || n > ZKHIP_MAX_PAIRS || (n && (!d_g1 || !d_g2))) { set_error("pairing_check: null pointer or more than %d pairs", ZKHIP_MAX_PAIRS); return ZKHIP_EINVAL; }
  // the kernel reads the pairs with 16-byte vector loads and stores the verdict as one 32-bit word
  if ((n && (((uintptr_t)d_g1 | (uintptr_t)d_g2) & 15)) || ((uintptr_t)d_ok & 3)) { set_error("pairing_check: d_g1 / d_g2 must be 16-byte aligned, d_ok 4-byte aligned"); return ZKHIP_EINVAL; }
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  return pairing_check_device((const uint32_t*)d_g1, (const uint32_t*)d_g2, n, (uint32_t*)d_ok, caller_stream(stream));
}

int zkhip_pairing_check(const uint64_t* g1, const uint64_t* g2, size_t n, int* ok) {
  ZK_API_RANGE();
  if (!ok || n > ZKHIP_MAX_PAIRS || (n && (!g1 || !g2))) { set_error("pairing_check: null pointer or more than %d pairs", ZKHIP_MAX_PAIRS); return ZKHIP_EINVAL; }
  lane_hold H;
  if (H.rc != ZKHIP_OK) return H.rc;
  int rc;
  hipStream_t s = H.s;
  if ((rc = H.sc->poly.reserve(ZKHIP_MAX_PAIRS * (64 + 128) + 64)) != ZKHIP_OK) return rc;
  char* d = (char*)H.sc->poly.p;                             // g1 | g2 | verdict
  if (n) {
    HIPCHK(hipMemcpyAsync(d, g1, n * 64, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d + ZKHIP_MAX_PAIRS * 64, g2, n * 128, hipMemcpyHostToDevice, s));
  }
  uint32_t* d_ok = (uint32_t*)(d + ZKHIP_MAX_PAIRS * (64 + 128));
  if ((rc = pairing_check_device((const uint32_t*)d, (const uint32_t*)(d + ZKHIP_MAX_PAIRS * 64), n, d_ok, s)) != ZKHIP_OK) return rc;
  HIPCHK(hipMemcpyAsync(H.L->pinned, d_ok, 4, hipMemcpyDeviceToHost, s));
  if ((rc = H.finish()) != ZKHIP_OK) return rc;
  *ok = *(const uint32_t*)H.L->pinned ? 1 : 0;
  return ZKHIP_OK;
}

int zkhip_test_fq12_op(int op, const uint64_t* a, const uint64_t* b, uint64_t* out) {
  ZK_API_RANGE();
  const int which = (op & 256) ? 1 : ((op & 512) ? 2 : 3), base_op = op & 255;
  if (op < 0 || (op & ~(255 | 256 | 512)) || base_op > 11 || !a || !b || !out) { set_error("test_fq12_op: bad argument"); return ZKHIP_EINVAL; }
  lane_hold H;
  if (H.rc != ZKHIP_OK) return H.rc;
  int rc;
  hipStream_t s = H.s;
  if ((rc = H.sc->poly.reserve(4 * 384)) != ZKHIP_OK) return rc;
  char* d = (char*)H.sc->poly.p;
  HIPCHK(hipMemcpyAsync(d, a, 384, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(d + 384, b, 384, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(d + 768, out, 768, hipMemcpyHostToDevice, s));       // the half that is not computed stays as the caller had it
  if ((rc = test_fq12_op(base_op, which, (const uint32_t*)d, (const uint32_t*)(d + 384), (uint32_t*)(d + 768), s)) != ZKHIP_OK) return rc;
  HIPCHK(hipMemcpyAsync(out, d + 768, 768, hipMemcpyDeviceToHost, s));
  return H.finish();
}

}  // extern "C"

// ---- Poseidon (include/zkhip.h, "Poseidon") ------------------------------------------------------------------------------------------------
namespace zkhip {
// the kernels' table on the primary device (g_mu held): uploaded once, on `s`, and waited for -- the source is host memory of this call
static int poseidon_device_table(hipStream_t s, const uint32_t** d_tab) {
  device_ctx& P = primary();
  if (!P.poseidon_table_ready) {
    const poseidon_tables& T = poseidon_tab();
    int rc;
    if ((rc = P.poseidon_table.reserve(sizeof(T.dev))) != ZKHIP_OK) return rc;
    HIPCHK(hipMemcpyAsync(P.poseidon_table.p, T.dev, sizeof(T.dev), hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    P.poseidon_table_ready = true;
  }
  *d_tab = (const uint32_t*)P.poseidon_table.p;
  return ZKHIP_OK;
}
}  // namespace zkhip

extern "C" {

int zkhip_poseidon_permute(uint64_t* states, size_t n) {
  if (n && !states) { set_error("poseidon_permute: null pointer"); return ZKHIP_EINVAL; }
  for (size_t i = 0; i < n; i++) {
    halo2::Fr st[3];
    memcpy(st, states + i * 12, 96);
    poseidon_host_permute(st);
    memcpy(states + i * 12, st, 96);
  }
  return ZKHIP_OK;
}

int zkhip_poseidon_hash(const uint64_t* fr, size_t n, uint64_t out[4]) {
  if (!out || (n && !fr)) { set_error("poseidon_hash: null pointer"); return ZKHIP_EINVAL; }
  if (n > 0xffffffffu) { set_error("poseidon_hash: more than 2^32 - 1 elements"); return ZKHIP_EINVAL; }
  const halo2::Fr h = poseidon_host_hash((const halo2::Fr*)fr, n);
  memcpy(out, h.l, 32);
  return ZKHIP_OK;
}

int zkhip_poseidon_constants(uint64_t out[204 * 4]) {
  if (!out) { set_error("poseidon_constants: null pointer"); return ZKHIP_EINVAL; }
  static_assert(POSEIDON_TAB_INIT == 204, "the header's count");
  memcpy(out, poseidon_tab().canon, (size_t)POSEIDON_TAB_INIT * 32);
  return ZKHIP_OK;
}

int zkhip_poseidon_hash_many_device(const void* d_in, size_t n, uint32_t width, void* d_out, void* stream) {
  ZK_API_RANGE();
  if (width < 1 || width > ZKHIP_POSEIDON_MAX_WIDTH) { set_error("poseidon_hash_many: width %u is not in 1..%d", width, ZKHIP_POSEIDON_MAX_WIDTH); return ZKHIP_EINVAL; }
  if (n && (!d_in || !d_out)) { set_error("poseidon_hash_many: null pointer"); return ZKHIP_EINVAL; }
  if (((uintptr_t)d_in | (uintptr_t)d_out) & 15) { set_error("poseidon_hash_many: d_in and d_out must be 16-byte aligned"); return ZKHIP_EINVAL; }
  if (n > ((size_t)1 << 30)) { set_error("poseidon_hash_many: more than 2^30 messages in one call"); return ZKHIP_EINVAL; }
  if (n == 0) return ZKHIP_OK;
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  hipStream_t s = caller_stream(stream);
  const uint32_t* d_tab = nullptr;
  if ((rc = poseidon_device_table(s, &d_tab)) != ZKHIP_OK) return rc;
  return poseidon_hash_many_device((const uint32_t*)d_in, n, width, (uint32_t*)d_out, d_tab, s);
}

int zkhip_poseidon_hash_points_device(const void* d_points, size_t n, uint32_t layout, void* d_out, void* stream) {
  ZK_API_RANGE();
  if (layout > 1) { set_error("poseidon_hash_points: layout %u is neither 0 (nullifier) nor 1 (member)", layout); return ZKHIP_EINVAL; }
  if (n && (!d_points || !d_out)) { set_error("poseidon_hash_points: null pointer"); return ZKHIP_EINVAL; }
  if (((uintptr_t)d_points | (uintptr_t)d_out) & 15) { set_error("poseidon_hash_points: d_points and d_out must be 16-byte aligned"); return ZKHIP_EINVAL; }
  if (n > ((size_t)1 << 30)) { set_error("poseidon_hash_points: more than 2^30 points in one call"); return ZKHIP_EINVAL; }
  if (n == 0) return ZKHIP_OK;
  const uintptr_t in = (uintptr_t)d_points, out = (uintptr_t)d_out;
  if (in < out + n * 32 && out < in + n * 64) { set_error("poseidon_hash_points: d_out overlaps d_points"); return ZKHIP_EINVAL; }
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  hipStream_t s = caller_stream(stream);
  const uint32_t* d_tab = nullptr;
  if ((rc = poseidon_device_table(s, &d_tab)) != ZKHIP_OK) return rc;
  return poseidon_hash_points_device((const uint32_t*)d_points, n, layout, (uint32_t*)d_out, d_tab, s);
}

int zkhip_poseidon_merkle_device(const void* d_leaves, size_t n_leaves, void* d_nodes, void* stream) {
  ZK_API_RANGE();
  if (n_leaves == 0 || (n_leaves & (n_leaves - 1)) || n_leaves > ((size_t)1 << 30)) {
    set_error("poseidon_merkle: %zu leaves: not a power of two in 1..2^30", n_leaves);
    return ZKHIP_EINVAL;
  }
  if (!d_leaves || (n_leaves > 1 && !d_nodes)) { set_error("poseidon_merkle: null pointer"); return ZKHIP_EINVAL; }
  if (((uintptr_t)d_leaves | (uintptr_t)d_nodes) & 15) { set_error("poseidon_merkle: d_leaves and d_nodes must be 16-byte aligned"); return ZKHIP_EINVAL; }
  if (n_leaves == 1) return ZKHIP_OK;
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  hipStream_t s = caller_stream(stream);
  scratch* sc = scratch_for(primary(), s);
  const uint32_t* d_tab = nullptr;
  if ((rc = poseidon_device_table(s, &d_tab)) != ZKHIP_OK) return rc;
  if ((rc = sc->small.reserve(poseidon_merkle_workspace(n_leaves))) != ZKHIP_OK) return rc;
  return poseidon_merkle_device((const uint32_t*)d_leaves, n_leaves, (uint32_t*)d_nodes, d_tab, sc->small.p, sc->small.cap, s);
}

}  // extern "C"

// ---- Paillier tally (include/zkhip.h, "Paillier tally") ------------------------------------------------------------------------------------------
// Every refusal is decided on the host before HIP is touched: a refused call enqueues nothing and works in a process that has no device.
namespace zkhip {
static bool pl_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return a_bytes && b_bytes && x < y + b_bytes && y < x + a_bytes;
}
static int pl_context(const char* who, const uint64_t* n, modn_ctx* ctx) {
  if (!n) { set_error("%s: null modulus", who); return ZKHIP_EINVAL; }
  if (!paillier_context(n, ctx)) { set_error("%s: n must be odd and at least 3 (Montgomery arithmetic mod n^2)", who); return ZKHIP_EINVAL; }
  return ZKHIP_OK;
}
constexpr size_t PL_MAX_COUNT = (size_t)1 << 32;          // ciphertexts of one call
constexpr size_t PL_BYTES = ZKHIP_PAILLIER_WORDS * 8;
}  // namespace zkhip

extern "C" {

int zkhip_paillier_mul_device(const uint64_t n[3], const void* d_a, const void* d_b, size_t count, void* d_out, void* stream) {
  ZK_API_RANGE();
  modn_ctx ctx;
  int rc = pl_context("paillier_mul", n, &ctx);
  if (rc != ZKHIP_OK) return rc;
  if (count > PL_MAX_COUNT) { set_error("paillier_mul: more than 2^32 ciphertexts in one call"); return ZKHIP_EINVAL; }
  if (count && (!d_a || !d_b || !d_out)) { set_error("paillier_mul: null pointer"); return ZKHIP_EINVAL; }
  if (count && (((uintptr_t)d_a | (uintptr_t)d_b | (uintptr_t)d_out) & 7)) { set_error("paillier_mul: pointers must be 8-byte aligned"); return ZKHIP_EINVAL; }
  if (count == 0) return ZKHIP_OK;
  // d_out may BE an input; a partial overlap would let one lane's store reach another lane's load
  for (const void* in : {d_a, d_b})
    if (in != d_out && pl_overlap(in, count * PL_BYTES, d_out, count * PL_BYTES)) { set_error("paillier_mul: d_out overlaps an input without being it"); return ZKHIP_EINVAL; }
  guard_t g(g_mu);
  if ((rc = ensure_init()) != ZKHIP_OK) return rc;
  return paillier_mul_device(ctx, (const uint64_t*)d_a, (const uint64_t*)d_b, count, (uint64_t*)d_out, caller_stream(stream));
}

int zkhip_paillier_tally_device(const uint64_t n[3], const void* d_ballots, size_t n_ballots, uint32_t n_cols, const void* d_init, void* d_running, void* stream) {
  ZK_API_RANGE();
  modn_ctx ctx;
  int rc = pl_context("paillier_tally", n, &ctx);
  if (rc != ZKHIP_OK) return rc;
  if (n_cols == 0) { set_error("paillier_tally: n_cols is 0"); return ZKHIP_EINVAL; }
  if (n_ballots >= PL_MAX_COUNT || (n_ballots + 1) * (size_t)n_cols > PL_MAX_COUNT) { set_error("paillier_tally: more than 2^32 ciphertexts in one call"); return ZKHIP_EINVAL; }
  if (!d_running || (n_ballots && !d_ballots)) { set_error("paillier_tally: null pointer"); return ZKHIP_EINVAL; }
  if (((uintptr_t)d_running | (uintptr_t)d_init | (n_ballots ? (uintptr_t)d_ballots : 0)) & 7) { set_error("paillier_tally: pointers must be 8-byte aligned"); return ZKHIP_EINVAL; }
  const size_t row = (size_t)n_cols * PL_BYTES;
  if (pl_overlap(d_running, (n_ballots + 1) * row, d_ballots, n_ballots * row) || (d_init && pl_overlap(d_running, (n_ballots + 1) * row, d_init, row))) {
    set_error("paillier_tally: d_running overlaps an input");
    return ZKHIP_EINVAL;
  }
  guard_t g(g_mu);
  if ((rc = ensure_init()) != ZKHIP_OK) return rc;
  hipStream_t s = caller_stream(stream);
  scratch* sc = scratch_for(primary(), s);
  if ((rc = sc->ws.reserve(paillier_tally_workspace_bytes(n_ballots, n_cols))) != ZKHIP_OK) return rc;
  return paillier_tally_device(ctx, (const uint64_t*)d_ballots, n_ballots, n_cols, (const uint64_t*)d_init, (uint64_t*)d_running, sc->ws.p, sc->ws.cap, s);
}

int zkhip_paillier_encrypt_device(const uint64_t n[3], const uint64_t g[6], const void* d_m, const void* d_r, size_t count, void* d_out, void* stream) {
  ZK_API_RANGE();
  modn_ctx ctx;
  int rc = pl_context("paillier_encrypt", n, &ctx);
  if (rc != ZKHIP_OK) return rc;
  if (!g) { set_error("paillier_encrypt: null base"); return ZKHIP_EINVAL; }
  if (count > PL_MAX_COUNT) { set_error("paillier_encrypt: more than 2^32 ciphertexts in one call"); return ZKHIP_EINVAL; }
  if (count && (!d_m || !d_r || !d_out)) { set_error("paillier_encrypt: null pointer"); return ZKHIP_EINVAL; }
  if (count && (((uintptr_t)d_m | (uintptr_t)d_r | (uintptr_t)d_out) & 7)) { set_error("paillier_encrypt: pointers must be 8-byte aligned"); return ZKHIP_EINVAL; }
  if (count == 0) return ZKHIP_OK;
  if (pl_overlap(d_out, count * PL_BYTES, d_m, count * 32) || pl_overlap(d_out, count * PL_BYTES, d_r, count * 24)) { set_error("paillier_encrypt: d_out overlaps an input"); return ZKHIP_EINVAL; }
  guard_t gd(g_mu);
  if ((rc = ensure_init()) != ZKHIP_OK) return rc;
  return paillier_encrypt_device(ctx, n, g, (const uint64_t*)d_m, (const uint64_t*)d_r, count, (uint64_t*)d_out, caller_stream(stream));
}

}  // extern "C"

// ---- PLUME nullifiers on secp256k1 (include/zkhip.h, "PLUME nullifiers on secp256k1") -----------------------------------------------------------
// Every refusal is decided on the host before HIP is touched: a refused call enqueues nothing and works in a process that has no device.
namespace zkhip {
struct pm_span {
  const void* p;
  size_t bytes;
  bool out;
};
constexpr size_t PM_MAX_COUNT = (size_t)1 << 30;
constexpr size_t PM_POINT = 64, PM_SCALAR = 32;
static int pm_message(const char* who, const uint8_t* msg, size_t msg_len, h2c_prefix* pre) {
  if (msg_len > ZKHIP_PLUME_MAX_MSG) { set_error("%s: the message is longer than ZKHIP_PLUME_MAX_MSG bytes", who); return ZKHIP_EINVAL; }
  if (msg_len && !msg) { set_error("%s: null message", who); return ZKHIP_EINVAL; }
  h2c_prefix_build(msg, msg_len, pre);
  return ZKHIP_OK;
}
// the arrays of a call: none null (count > 0), all 8-byte aligned, no output overlapping anything else
static int pm_arrays(const char* who, size_t count, const pm_span* spans, int n) {
  if (count > PM_MAX_COUNT) { set_error("%s: more than 2^30 elements in one call", who); return ZKHIP_EINVAL; }
  for (int i = 0; i < n; i++) {
    if (count && !spans[i].p) { set_error("%s: null pointer", who); return ZKHIP_EINVAL; }
    if ((uintptr_t)spans[i].p & 7) { set_error("%s: pointers must be 8-byte aligned", who); return ZKHIP_EINVAL; }
  }
  for (int i = 0; i < n; i++)
    for (int j = 0; j < n; j++)
      if (i != j && spans[i].out && pl_overlap(spans[i].p, spans[i].bytes, spans[j].p, spans[j].bytes)) { set_error("%s: an output overlaps another array", who); return ZKHIP_EINVAL; }
  return ZKHIP_OK;
}
static sk_aff pm_point(const uint64_t* w) {
  sk_aff a;
  a.x = sk_from_words(w);
  a.y = sk_from_words(w + 4);
  return a;
}
}  // namespace zkhip

extern "C" {

int zkhip_secp256k1_lincomb_device(const void* d_a, const void* d_p, const void* d_b, const void* d_q, size_t count, void* d_out, void* d_status, void* stream) {
  ZK_API_RANGE();
  const pm_span spans[] = {{d_a, count * PM_SCALAR, false}, {d_p, count * PM_POINT, false}, {d_b, count * PM_SCALAR, false}, {d_q, count * PM_POINT, false},
                           {d_out, count * PM_POINT, true}, {d_status, count * 4, true}};
  int rc = pm_arrays("secp256k1_lincomb", count, spans, 6);
  if (rc != ZKHIP_OK || count == 0) return rc;
  guard_t g(g_mu);
  if ((rc = ensure_init()) != ZKHIP_OK) return rc;
  return secp256k1_lincomb_device((const uint64_t*)d_a, (const uint64_t*)d_p, (const uint64_t*)d_b, (const uint64_t*)d_q, count, (uint64_t*)d_out, (uint32_t*)d_status,
                                  caller_stream(stream));
}

int zkhip_secp256k1_hash_to_curve_device(const uint8_t* msg, size_t msg_len, const void* d_pk, size_t count, void* d_out, void* d_status, void* stream) {
  ZK_API_RANGE();
  h2c_prefix pre;
  int rc = pm_message("secp256k1_hash_to_curve", msg, msg_len, &pre);
  if (rc != ZKHIP_OK) return rc;
  const pm_span spans[] = {{d_pk, count * PM_POINT, false}, {d_out, count * PM_POINT, true}, {d_status, count * 4, true}};
  rc = pm_arrays("secp256k1_hash_to_curve", count, spans, 3);
  if (rc != ZKHIP_OK || count == 0) return rc;
  guard_t g(g_mu);
  if ((rc = ensure_init()) != ZKHIP_OK) return rc;
  return secp256k1_hash_to_curve_device(pre, (const uint64_t*)d_pk, count, (uint64_t*)d_out, (uint32_t*)d_status, caller_stream(stream));
}

int zkhip_plume_verify_device(const uint8_t* msg, size_t msg_len, const void* d_pk, const void* d_nullifier, const void* d_s, const void* d_c, size_t count, void* d_status,
                              void* d_report, void* d_h_out, void* stream) {
  ZK_API_RANGE();
  h2c_prefix pre;
  int rc = pm_message("plume_verify", msg, msg_len, &pre);
  if (rc != ZKHIP_OK) return rc;
  if (!d_report) { set_error("plume_verify: null report"); return ZKHIP_EINVAL; }
  const pm_span spans[] = {{d_pk, count * PM_POINT, false}, {d_nullifier, count * PM_POINT, false}, {d_s, count * PM_SCALAR, false}, {d_c, count * PM_SCALAR, false},
                           {d_status, count * 4, true}, {d_report, sizeof(zkhip_check_report), true}, {d_h_out, count * PM_POINT, true}};
  rc = pm_arrays("plume_verify", count, spans, d_h_out ? 7 : 6);
  if (rc != ZKHIP_OK) return rc;
  guard_t g(g_mu);
  if ((rc = ensure_init()) != ZKHIP_OK) return rc;
  return plume_verify_device(pre, (const uint64_t*)d_pk, (const uint64_t*)d_nullifier, (const uint64_t*)d_s, (const uint64_t*)d_c, count, (uint32_t*)d_status, d_report,
                             (uint64_t*)d_h_out, caller_stream(stream));
}

int zkhip_plume_sign_device(const uint8_t* msg, size_t msg_len, const void* d_sk, const void* d_r, size_t count, void* d_pk, void* d_nullifier, void* d_s, void* d_c,
                            void* d_status, void* d_h_out, void* stream) {
  ZK_API_RANGE();
  h2c_prefix pre;
  int rc = pm_message("plume_sign", msg, msg_len, &pre);
  if (rc != ZKHIP_OK) return rc;
  const pm_span spans[] = {{d_sk, count * PM_SCALAR, false}, {d_r, count * PM_SCALAR, false}, {d_pk, count * PM_POINT, true}, {d_nullifier, count * PM_POINT, true},
                           {d_s, count * PM_SCALAR, true}, {d_c, count * PM_SCALAR, true}, {d_status, count * 4, true}, {d_h_out, count * PM_POINT, true}};
  rc = pm_arrays("plume_sign", count, spans, d_h_out ? 8 : 7);
  if (rc != ZKHIP_OK || count == 0) return rc;
  guard_t g(g_mu);
  if ((rc = ensure_init()) != ZKHIP_OK) return rc;
  return plume_sign_device(pre, (const uint64_t*)d_sk, (const uint64_t*)d_r, count, (uint64_t*)d_pk, (uint64_t*)d_nullifier, (uint64_t*)d_s, (uint64_t*)d_c,
                           (uint32_t*)d_status, (uint64_t*)d_h_out, caller_stream(stream));
}

int zkhip_plume_sign(const uint8_t* msg, size_t msg_len, const uint64_t sk[4], const uint64_t r[4], uint64_t pk[8], uint64_t nullifier[8], uint64_t s[4], uint64_t c[4],
                     uint32_t* status, uint64_t h_out[8]) {
  h2c_prefix pre;
  const int rc = pm_message("plume_sign", msg, msg_len, &pre);
  if (rc != ZKHIP_OK) return rc;
  if (!sk || !r || !pk || !nullifier || !s || !c || !status) { set_error("plume_sign: null pointer"); return ZKHIP_EINVAL; }
  plume_signature sig;
  *status = plume_sign(pre, sk_from_words(sk), sk_from_words(r), &sig);
  sk_to_words(sig.pk.x, pk);
  sk_to_words(sig.pk.y, pk + 4);
  sk_to_words(sig.nullifier.x, nullifier);
  sk_to_words(sig.nullifier.y, nullifier + 4);
  sk_to_words(sig.s, s);
  sk_to_words(sig.c, c);
  if (h_out) {
    sk_to_words(sig.h.x, h_out);
    sk_to_words(sig.h.y, h_out + 4);
  }
  return ZKHIP_OK;
}

int zkhip_secp256k1_hash_to_curve(const uint8_t* msg, size_t msg_len, const uint64_t pk[8], uint64_t out[8], uint32_t* status) {
  h2c_prefix pre;
  const int rc = pm_message("secp256k1_hash_to_curve", msg, msg_len, &pre);
  if (rc != ZKHIP_OK) return rc;
  if (!pk || !out || !status) { set_error("secp256k1_hash_to_curve: null pointer"); return ZKHIP_EINVAL; }
  const sk_aff key = pm_point(pk);
  const bool ok = sk_on_curve(key);
  sk_aff h;
  h.x = h.y = sk_small(0);
  if (ok) h = h2c_hash(pre, key);
  sk_to_words(h.x, out);
  sk_to_words(h.y, out + 4);
  *status = ok ? PLUME_OK : PLUME_MALFORMED;
  return ZKHIP_OK;
}

int zkhip_plume_verify(const uint8_t* msg, size_t msg_len, const uint64_t pk[8], const uint64_t nullifier[8], const uint64_t s[4], const uint64_t c[4], uint32_t* verdict,
                       uint64_t h_out[8]) {
  h2c_prefix pre;
  const int rc = pm_message("plume_verify", msg, msg_len, &pre);
  if (rc != ZKHIP_OK) return rc;
  if (!pk || !nullifier || !s || !c || !verdict) { set_error("plume_verify: null pointer"); return ZKHIP_EINVAL; }
  sk_aff h;
  *verdict = plume_verdict(pre, pm_point(pk), pm_point(nullifier), sk_from_words(s), sk_from_words(c), &h);
  if (h_out) {
    sk_to_words(h.x, h_out);
    sk_to_words(h.y, h_out + 4);
  }
  return ZKHIP_OK;
}

}  // extern "C"

// ---- indexed Merkle tree (include/zkhip.h, "indexed Merkle tree") -----------------------------------------------------------------------------
// The object owns the tree in device memory (primary device), the ordered index of the used values (imt.hpp, host), a grow-only workspace and
// a pinned staging block for what a batch uploads; `staged` says when the last batch's uploads have left the block.
struct zkhip_imt {
  uint32_t depth = 0;
  zkhip::imt_index index;
  uint32_t *leaves = nullptr, *nodes = nullptr, *preimages = nullptr;
  zkhip::dev_buf ws;
  void* stage = nullptr;
  size_t stage_cap = 0;
  hipEvent_t staged = nullptr;
  bool staged_live = false;
  hipStream_t last = nullptr;          // the stream of the last insert: the read-backs run behind it
  size_t n_leaves() const { return (size_t)1 << depth; }
};

namespace zkhip {
static void imt_release(zkhip_imt* t) {
  if (t->staged) { if (t->staged_live) (void)hipEventSynchronize(t->staged); (void)hipEventDestroy(t->staged); }
  if (t->stage) (void)hipHostFree(t->stage);
  t->ws.release();
  if (t->leaves) (void)hipFree(t->leaves);
  if (t->nodes) (void)hipFree(t->nodes);
  if (t->preimages) (void)hipFree(t->preimages);
  delete t;
}
static inline halo2::Fr imt_fr_of_index(uint32_t j) { return halo2::detail::from_u64(j); }
}  // namespace zkhip

extern "C" {

int zkhip_imt_link(const uint64_t* used_vals, size_t n_used, const uint64_t* new_vals, size_t n_new, uint32_t* low_index_out, size_t* first_bad) {
  if (first_bad) *first_bad = (size_t)-1;
  if ((n_used && !used_vals) || (n_new && (!new_vals || !low_index_out))) { set_error("imt_link: null pointer"); return ZKHIP_EINVAL; }
  if (n_used > 0xffffffffu || n_new > 0xffffffffu - (n_used ? n_used : 1)) { set_error("imt_link: more than 2^32 - 1 leaves"); return ZKHIP_EINVAL; }
  if (n_used && (used_vals[0] | used_vals[1] | used_vals[2] | used_vals[3])) { set_error("imt_link: leaf 0 is the head: its value is 0"); return ZKHIP_EINVAL; }
  imt_index index;
  const char* why = nullptr;
  size_t bad = 0;
  if (n_used > 1 && !index.link(used_vals + 4, n_used - 1, (size_t)-1, nullptr, &bad, &why)) {
    set_error("imt_link: used value %zu: %s", bad + 1, why);
    return ZKHIP_EINVAL;
  }
  std::vector<imt_link> links(n_new);
  if (!index.link(new_vals, n_new, (size_t)-1, links.data(), &bad, &why)) {
    if (first_bad) *first_bad = bad;
    set_error("imt_link: new value %zu: %s", bad, why);
    return ZKHIP_EINVAL;
  }
  for (size_t i = 0; i < n_new; i++) low_index_out[i] = links[i].low;
  return ZKHIP_OK;
}

int zkhip_imt_create(uint32_t depth, zkhip_imt** out) {
  ZK_API_RANGE();
  if (!out) { set_error("imt_create: null pointer"); return ZKHIP_EINVAL; }
  *out = nullptr;
  if (depth < 1 || depth > ZKHIP_IMT_MAX_DEPTH) { set_error("imt_create: depth %u is not in 1..%d", depth, ZKHIP_IMT_MAX_DEPTH); return ZKHIP_EINVAL; }
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  zkhip_imt* t = new (std::nothrow) zkhip_imt();
  if (!t) { set_error("imt_create: out of memory"); return ZKHIP_ENOMEM; }
  t->depth = depth;
  const size_t n = t->n_leaves();
  if (hipMalloc((void**)&t->leaves, n * 32) != hipSuccess || hipMalloc((void**)&t->nodes, (n - 1) * 32) != hipSuccess ||
      hipMalloc((void**)&t->preimages, n * 96) != hipSuccess || hipEventCreateWithFlags(&t->staged, hipEventDisableTiming) != hipSuccess) {
    (void)hipGetLastError();
    imt_release(t);
    set_error("imt_create: no device memory for a tree of depth %u", depth);
    return ZKHIP_ENOMEM;
  }
  // the empty tree: every level one repeated value, depth + 1 host hashes
  const uint32_t* d_tab = nullptr;
  rc = poseidon_device_table(nullptr, &d_tab);
  halo2::Fr h = poseidon_host_hash(std::vector<halo2::Fr>(3, halo2::Fr{{0, 0, 0, 0}}).data(), 3);
  if (rc == ZKHIP_OK && hipMemsetAsync(t->preimages, 0, n * 96, nullptr) != hipSuccess) { set_error("imt_create: memset failed"); rc = ZKHIP_EHIP; }
  for (uint32_t L = 0; L <= depth && rc == ZKHIP_OK; L++) {
    uint32_t w[8];
    memcpy(w, h.l, 32);
    rc = imt_fill_device(L == 0 ? t->leaves : t->nodes + (n - (n >> (L - 1))) * 8, n >> L, w, nullptr);
    const halo2::Fr two[2] = {h, h};
    h = poseidon_host_hash(two, 2);
  }
  if (rc == ZKHIP_OK && hipStreamSynchronize(nullptr) != hipSuccess) { set_error("imt_create: the fills failed"); rc = ZKHIP_EHIP; }
  if (rc != ZKHIP_OK) { imt_release(t); return rc; }
  *out = t;
  return ZKHIP_OK;
}

int zkhip_imt_destroy(zkhip_imt* t) {
  ZK_API_RANGE();
  if (!t) return ZKHIP_OK;
  guard_t g(g_mu);
  if (g_ctx.ready) (void)ensure_init();
  imt_release(t);                      // hipFree waits for the device: nothing queued still reads the tree
  return ZKHIP_OK;
}

int zkhip_imt_size(const zkhip_imt* t, uint32_t* depth, uint32_t* used) {
  if (!t) { set_error("imt_size: null tree"); return ZKHIP_EINVAL; }
  if (depth) *depth = t->depth;
  if (used) *used = (uint32_t)t->index.used();
  return ZKHIP_OK;
}

int zkhip_imt_insert(zkhip_imt* t, const uint64_t* values, size_t n_new, const zkhip_imt_witness* out, size_t* first_bad, void* stream) {
  ZK_API_RANGE();
  if (first_bad) *first_bad = (size_t)-1;
  if (!t || (n_new && !values)) { set_error("imt_insert: null pointer"); return ZKHIP_EINVAL; }
  if (out) {
    if (n_new && (!out->d_roots || !out->d_low_leaves || !out->d_new_leaves || !out->d_low_indices || !out->d_low_proofs || !out->d_new_proofs)) {
      set_error("imt_insert: a null pointer in the witness buffers");
      return ZKHIP_EINVAL;
    }
    if ((((uintptr_t)out->d_roots | (uintptr_t)out->d_low_leaves | (uintptr_t)out->d_new_leaves | (uintptr_t)out->d_low_proofs | (uintptr_t)out->d_new_proofs) & 15) ||
        ((uintptr_t)out->d_low_indices & 3)) {
      set_error("imt_insert: the witness buffers must be 16-byte aligned (d_low_indices: 4-byte)");
      return ZKHIP_EINVAL;
    }
  }
  if (n_new == 0) return ZKHIP_OK;
  const size_t used0 = t->index.used(), n = t->n_leaves();
  std::vector<imt_link> links(n_new);
  const char* why = nullptr;
  size_t bad = 0;
  if (!t->index.link(values, n_new, n, links.data(), &bad, &why)) {
    if (first_bad) *first_bad = bad;
    set_error("imt_insert: value %zu: %s", bad, why);
    return ZKHIP_EINVAL;
  }
  guard_t g(g_mu);
  int rc = ensure_init();
  hipStream_t s = caller_stream(stream);
  const uint32_t* d_tab = nullptr;
  if (rc == ZKHIP_OK) rc = poseidon_device_table(s, &d_tab);
  const size_t n_ev = 2 * n_new, up_bytes = n_ev * (8 + 96), stage_bytes = up_bytes + n_new * (96 + 4);
  if (rc == ZKHIP_OK) rc = t->ws.reserve(imt_workspace_bytes(n_new));
  if (rc == ZKHIP_OK && t->staged_live && hipEventSynchronize(t->staged) != hipSuccess) { set_error("imt_insert: the last batch's uploads failed"); rc = ZKHIP_EHIP; }
  if (rc == ZKHIP_OK && stage_bytes > t->stage_cap) {
    if (t->stage) (void)hipHostFree(t->stage);
    t->stage = nullptr; t->stage_cap = 0;
    if (hipHostMalloc(&t->stage, stage_bytes + stage_bytes / 8, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); t->stage = nullptr; set_error("imt_insert: no pinned memory (%zu bytes)", stage_bytes); rc = ZKHIP_ENOMEM; }
    else t->stage_cap = stage_bytes + stage_bytes / 8;
  }
  if (rc != ZKHIP_OK) { t->index.unlink(n_new); return rc; }
  // the events: time 2 i the low leaf as insertion i leaves it, time 2 i + 1 the new leaf; keys ordered by (leaf, time) for level 0
  uint64_t* keys = (uint64_t*)t->stage;
  halo2::Fr* pre = (halo2::Fr*)((char*)t->stage + n_ev * 8);
  halo2::Fr* low_before = (halo2::Fr*)((char*)t->stage + up_bytes);
  uint32_t* low_idx = (uint32_t*)((char*)t->stage + up_bytes + n_new * 96);
  for (size_t i = 0; i < n_new; i++) {
    const imt_link& k = links[i];
    const uint32_t j = (uint32_t)(used0 + i);
    const halo2::Fr next_idx = imt_fr_of_index(k.next_idx);
    halo2::Fr v;
    memcpy(v.l, values + 4 * i, 32);
    low_before[3 * i] = k.low_val; low_before[3 * i + 1] = k.next_val; low_before[3 * i + 2] = next_idx;
    pre[6 * i] = k.low_val; pre[6 * i + 1] = v; pre[6 * i + 2] = imt_fr_of_index(j);
    pre[6 * i + 3] = v; pre[6 * i + 4] = k.next_val; pre[6 * i + 5] = next_idx;
    low_idx[i] = k.low;
    keys[2 * i] = ((uint64_t)k.low << 32) | (uint64_t)(2 * i);
    keys[2 * i + 1] = ((uint64_t)j << 32) | (uint64_t)(2 * i + 1);
  }
  std::sort(keys, keys + n_ev);
  // from here on a failure leaves the stream and the tree in an unknown state (ZKHIP_EHIP): the index stays advanced, as the stream's work is
  HIPCHK(hipMemcpyAsync(t->ws.p, t->stage, up_bytes, hipMemcpyHostToDevice, s));
  if (out) {
    HIPCHK(hipMemcpyAsync(out->d_low_leaves, low_before, n_new * 96, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(out->d_low_indices, low_idx, n_new * 4, hipMemcpyHostToDevice, s));
  }
  HIPCHK(hipEventRecord(t->staged, s));
  t->staged_live = true;
  t->last = s;
  return imt_insert_device(t->depth, n_new, t->ws.p, t->leaves, t->nodes, t->preimages, out ? (uint32_t*)out->d_roots : nullptr, out ? (uint32_t*)out->d_new_leaves : nullptr,
                           out ? (uint32_t*)out->d_low_proofs : nullptr, out ? (uint32_t*)out->d_new_proofs : nullptr, d_tab, s);
}

// a handful of cells to the host behind the last insert: `cells` (pointer, bytes) pairs, copied in order into `out`
static int imt_read_back(zkhip_imt* t, const std::vector<std::pair<const void*, size_t>>& cells, uint64_t* out) {
  hipStream_t s;
  {
    guard_t g(g_mu);
    int rc = ensure_init();
    if (rc != ZKHIP_OK) return rc;
    s = t->last;
    char* at = (char*)out;
    for (auto& c : cells) { HIPCHK(hipMemcpyAsync(at, c.first, c.second, hipMemcpyDeviceToHost, s)); at += c.second; }
  }
  HIPCHK(hipStreamSynchronize(s));
  return ZKHIP_OK;
}

int zkhip_imt_root(zkhip_imt* t, uint64_t out[4]) {
  ZK_API_RANGE();
  if (!t || !out) { set_error("imt_root: null pointer"); return ZKHIP_EINVAL; }
  return imt_read_back(t, {{t->nodes + (t->n_leaves() - 2) * 8, 32}}, out);
}

int zkhip_imt_leaf(zkhip_imt* t, uint32_t index, uint64_t out[12]) {
  ZK_API_RANGE();
  if (!t || !out) { set_error("imt_leaf: null pointer"); return ZKHIP_EINVAL; }
  if (index >= t->n_leaves()) { set_error("imt_leaf: leaf %u of a tree of depth %u", index, t->depth); return ZKHIP_EINVAL; }
  return imt_read_back(t, {{t->preimages + (size_t)index * 24, 96}}, out);
}

int zkhip_imt_proof(zkhip_imt* t, uint32_t index, uint64_t* out) {
  ZK_API_RANGE();
  if (!t || !out) { set_error("imt_proof: null pointer"); return ZKHIP_EINVAL; }
  const size_t n = t->n_leaves();
  if (index >= n) { set_error("imt_proof: leaf %u of a tree of depth %u", index, t->depth); return ZKHIP_EINVAL; }
  std::vector<std::pair<const void*, size_t>> cells;
  for (uint32_t L = 0; L < t->depth; L++) {
    const uint32_t* level = L == 0 ? t->leaves : t->nodes + (n - (n >> (L - 1))) * 8;
    cells.push_back({level + (size_t)((index >> L) ^ 1u) * 8, 32});
  }
  return imt_read_back(t, cells, out);
}

int zkhip_imt_export_device(zkhip_imt* t, void* d_leaves, void* d_nodes, void* d_preimages, void* stream) {
  ZK_API_RANGE();
  if (!t || !d_leaves || !d_nodes || !d_preimages) { set_error("imt_export: null pointer"); return ZKHIP_EINVAL; }
  if (((uintptr_t)d_leaves | (uintptr_t)d_nodes | (uintptr_t)d_preimages) & 15) { set_error("imt_export: the buffers must be 16-byte aligned"); return ZKHIP_EINVAL; }
  guard_t g(g_mu);
  int rc = ensure_init();
  if (rc != ZKHIP_OK) return rc;
  hipStream_t s = caller_stream(stream);
  const size_t n = t->n_leaves();
  HIPCHK(hipMemcpyAsync(d_leaves, t->leaves, n * 32, hipMemcpyDeviceToDevice, s));
  HIPCHK(hipMemcpyAsync(d_nodes, t->nodes, (n - 1) * 32, hipMemcpyDeviceToDevice, s));
  HIPCHK(hipMemcpyAsync(d_preimages, t->preimages, n * 96, hipMemcpyDeviceToDevice, s));
  return ZKHIP_OK;
}

}  // extern "C"

// ---- transcript (include/zkhip.h, "transcript"): Blake2bWrite / Blake2bRead with Challenge255, or the Poseidon transcript ------------------------
// The object is host state: the hash, the proof bytes, a cursor, and a pinned staging block for the `_device` calls.  The calls marked "host" in
// the header never reach ensure_init(): their field arithmetic is zkhip::halo2::detail's 4 x 64 Montgomery product.
struct zkhip_transcript {
  bool poseidon = false;               // which hash absorbs: `st` (Blake2b) or `sponge`; everything else is common to both
  zkhip::poseidon_sponge* sponge = nullptr;
  zkhip::blake2b st;
  std::vector<uint8_t> proof;
  size_t cursor = 0;
  bool reader = false;
  int layout = 0;
  void* pinned = nullptr;              // hipHostMalloc, grown on demand by the `_device` calls
  size_t pinned_cap = 0;
};

namespace zkhip {
namespace hd = halo2::detail;

constexpr size_t TR_HEAD = 256;        // bytes in front of the payload in scratch::transcript
constexpr size_t TR_MAX = (size_t)1 << 24;

static const uint64_t RAW_ONE_64[4] = {1, 0, 0, 0};
// host byte order is little-endian (as everywhere in this library: the external formats are memcpy'd limbs)
static void fr_mont_to_repr(const uint64_t m[4], uint8_t out[32]) { uint64_t c[4]; hd::mont_mul(c, m, RAW_ONE_64, hd::R_MOD, hd::R_INV); memcpy(out, c, 32); }
static void fq_mont_to_repr(const uint64_t m[4], uint8_t out[32]) { uint64_t c[4]; hd::mont_mul(c, m, RAW_ONE_64, hd::Q_MOD, hd::Q_INV); memcpy(out, c, 32); }
static bool fr_repr_to_mont(const uint8_t in[32], uint64_t out[4]) {
  uint64_t v[4];
  memcpy(v, in, 32);
  if (hd::geq(v, hd::R_MOD)) return false;
  hd::mont_mul(out, v, hd::R_R2, hd::R_MOD, hd::R_INV);
  return true;
}
// 64 bytes as a little-endian integer lo + 2^256 hi, mod r, in Montgomery form: lo R + hi R^2 = mont(lo, R^2) + mont(hi, R^3)
// (the Montgomery product accepts one factor below 2^256 when the other is below r: the result is below 2r before its one subtraction)
static void fr_reduce512(const uint8_t in[64], uint64_t out[4]) {
  uint64_t lo[4], hi[4], r3[4];
  memcpy(lo, in, 32);
  memcpy(hi, in + 32, 32);
  hd::mont_mul(r3, hd::R_R2, hd::R_R2, hd::R_MOD, hd::R_INV);
  halo2::Fr a, b;
  hd::mont_mul(a.l, lo, hd::R_R2, hd::R_MOD, hd::R_INV);
  hd::mont_mul(b.l, hi, r3, hd::R_MOD, hd::R_INV);
  const halo2::Fr sum = hd::add_fr(a, b);
  memcpy(out, sum.l, 32);
}

// Poseidon: a canonical 32-byte integer below 2 r (a scalar, or an Fq coordinate: q < 2 r) into the sponge's buffer, mod r
static void tr_sponge_absorb(zkhip_transcript* t, const uint8_t repr[32]) {
  uint64_t v[4];
  memcpy(v, repr, 32);
  if (hd::geq(v, hd::R_MOD)) hd::sub(v, v, hd::R_MOD);
  t->sponge->update(hd::from_raw(v));
}
static void tr_absorb_scalar(zkhip_transcript* t, const uint8_t repr[32]) {
  if (t->poseidon) { tr_sponge_absorb(t, repr); return; }
  uint8_t b[33];
  b[0] = 0x02;
  memcpy(b + 1, repr, 32);
  t->st.update(b, 33);
}
static void tr_absorb_point(zkhip_transcript* t, const uint8_t xy[64]) {
  if (t->poseidon) { tr_sponge_absorb(t, xy); tr_sponge_absorb(t, xy + 32); return; }
  uint8_t b[65];
  b[0] = 0x01;
  memcpy(b + 1, xy, 64);
  t->st.update(b, 65);
}
static bool bytes_zero(const uint8_t* p, size_t n) { for (size_t i = 0; i < n; i++) if (p[i]) return false; return true; }

static int tr_pinned(zkhip_transcript* t, size_t bytes) {
  if (bytes <= t->pinned_cap) return ZKHIP_OK;
  if (t->pinned) (void)hipHostFree(t->pinned);
  t->pinned = nullptr; t->pinned_cap = 0;
  const size_t want = bytes + bytes / 2 + 4096;
  if (hipHostMalloc(&t->pinned, want, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); t->pinned = nullptr; set_error("transcript: hipHostMalloc(%zu) failed", want); return ZKHIP_ENOMEM; }
  t->pinned_cap = want;
  return ZKHIP_OK;
}
// the scratch set's record buffer with room for `payload` bytes behind the head
static int tr_reserve(scratch* sc, size_t payload) { return sc->transcript.reserve(TR_HEAD + payload); }
// A scratch set resolved under g_mu and then used WITHOUT it: the transcript's `_device` calls wait for the caller's stream -- all of the
// caller's earlier work, the MSMs that made the commitments included -- and hash on the host, and no other thread's call should stand
// behind that.  While pinned the set is not evicted (scratch_for) and zkhip_shutdown waits for it.  One stream, one enqueuing thread at a
// time (include/zkhip.h), so the set has one user.
struct scratch_pin {
  scratch* sc = nullptr;
  int rc = ZKHIP_OK;
  explicit scratch_pin(hipStream_t s) {
    std::lock_guard<std::recursive_mutex> g(g_mu);
    if ((rc = ensure_init()) != ZKHIP_OK) return;
    sc = scratch_for(primary(), s);
    sc->pins++;
  }
  ~scratch_pin() {
    if (!sc) return;
    std::lock_guard<std::recursive_mutex> g(g_mu);
    sc->pins--;
    g_lane_cv.notify_all();
  }
  scratch_pin(const scratch_pin&) = delete;
  scratch_pin& operator=(const scratch_pin&) = delete;
};
// The failure guard of the `_device` transcript calls, the lanes' rule on a caller's stream: a call that returns without
// done() -- any error after its first enqueue -- waits for the stream first, so that no copy into the transcript's pinned block is left queued.
struct stream_drain {
  hipStream_t s;
  bool armed = true;
  explicit stream_drain(hipStream_t st) : s(st) {}
  void done() { armed = false; }
  ~stream_drain() { if (armed) { (void)hipStreamSynchronize(s); (void)hipGetLastError(); } }
};

// one launch, one copy into the pinned block, one wait; then the host absorbs and appends.  The caller drains `s` on a non-OK return.
static int tr_write_points_core(zkhip_transcript* t, scratch* sc, hipStream_t s, const void* d_points, size_t n) {
  int rc;
  if ((rc = tr_reserve(sc, n * 96)) != ZKHIP_OK) return rc;
  if ((rc = tr_pinned(t, TR_HEAD + n * 96)) != ZKHIP_OK) return rc;
  char* d = (char*)sc->transcript.p;
  *(uint32_t*)t->pinned = 0;                               // the call's identity count starts at zero: no state is carried between calls
  HIPCHK(hipMemcpyAsync(d, t->pinned, 4, hipMemcpyHostToDevice, s));
  if ((rc = transcript_points_device((const uint32_t*)d_points, n, (uint32_t*)(d + TR_HEAD), t->layout, (uint32_t*)d, s)) != ZKHIP_OK) return rc;
  HIPCHK(hipMemcpyAsync(t->pinned, d, TR_HEAD + n * 96, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  const uint8_t* rec = (const uint8_t*)t->pinned + TR_HEAD;
  const uint32_t identities = *(const uint32_t*)t->pinned;
  if (identities) {
    size_t first = 0;
    while (first < n && !bytes_zero(rec + first * 96, 64)) first++;      // an identity input's record is zeros; no curve point has x = y = 0
    set_error("transcript: cannot write points at infinity to the transcript (point %zu of %zu; %u in all)", first, n, identities);
    return ZKHIP_EINVAL;
  }
  t->proof.reserve(t->proof.size() + n * 32);
  for (size_t i = 0; i < n; i++) {
    tr_absorb_point(t, rec + i * 96);
    t->proof.insert(t->proof.end(), rec + i * 96 + 64, rec + i * 96 + 96);
  }
  return ZKHIP_OK;
}

static int tr_write_scalars_core(zkhip_transcript* t, scratch* sc, hipStream_t s, const void* d_fr, size_t n) {
  int rc;
  if ((rc = tr_reserve(sc, n * 32)) != ZKHIP_OK) return rc;
  if ((rc = tr_pinned(t, n * 32)) != ZKHIP_OK) return rc;
  char* d = (char*)sc->transcript.p + TR_HEAD;
  if ((rc = transcript_scalars_device((const uint32_t*)d_fr, n, (uint32_t*)d, s)) != ZKHIP_OK) return rc;
  HIPCHK(hipMemcpyAsync(t->pinned, d, n * 32, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  const uint8_t* rec = (const uint8_t*)t->pinned;
  for (size_t i = 0; i < n; i++) tr_absorb_scalar(t, rec + i * 32);
  t->proof.insert(t->proof.end(), rec, rec + n * 32);
  return ZKHIP_OK;
}

// payload: encodings (32 n) | first_bad (64 bytes) | canonical x | y records (64 n).  host_out (nullable): the affine points, downloaded
// before anything is absorbed.
static int tr_read_points_core(zkhip_transcript* t, scratch* sc, hipStream_t s, size_t n, void* d_affine, uint64_t* host_out) {
  int rc;
  const size_t enc = n * 32, payload = enc + 64 + n * 64;
  if ((rc = tr_reserve(sc, payload)) != ZKHIP_OK) return rc;
  if ((rc = tr_pinned(t, payload)) != ZKHIP_OK) return rc;
  char* d = (char*)sc->transcript.p + TR_HEAD;
  uint8_t* pin = (uint8_t*)t->pinned;
  memcpy(pin, t->proof.data() + t->cursor, enc);
  memset(pin + enc, 0, 64);
  *(unsigned long long*)(pin + enc) = (unsigned long long)n;
  HIPCHK(hipMemcpyAsync(d, pin, enc + 64, hipMemcpyHostToDevice, s));
  unsigned long long* d_bad = (unsigned long long*)(d + enc);
  if ((rc = g1_decompress_device((const uint32_t*)d, n, (uint32_t*)d_affine, t->layout, d_bad, s)) != ZKHIP_OK) return rc;
  if ((rc = transcript_affine_device((const uint32_t*)d_affine, n, (uint32_t*)(d + enc + 64), d_bad, s)) != ZKHIP_OK) return rc;
  HIPCHK(hipMemcpyAsync(pin + enc, d + enc, 64 + n * 64, hipMemcpyDeviceToHost, s));
  if (host_out) HIPCHK(hipMemcpyAsync(host_out, d_affine, n * 64, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  const unsigned long long bad = *(const unsigned long long*)(pin + enc);
  if (bad < n) {
    set_error("transcript: read_points: encoding %llu of %zu (proof byte %zu) is not a point a transcript accepts (x not canonical, not on the curve, or the identity)",
              bad, n, t->cursor + (size_t)bad * 32);
    return ZKHIP_EINVAL;
  }
  for (size_t i = 0; i < n; i++) tr_absorb_point(t, pin + enc + 64 + i * 64);
  t->cursor += enc;
  return ZKHIP_OK;
}

static int tr_check_write(const zkhip_transcript* t, const void* p, size_t n, const char* who) {
  if (!t || (n && !p)) { set_error("%s: null pointer", who); return ZKHIP_EINVAL; }
  if (t->reader) { set_error("%s: this transcript reads a proof", who); return ZKHIP_EINVAL; }
  if (n > TR_MAX) { set_error("%s: more than 2^24 elements in one call", who); return ZKHIP_EINVAL; }
  return ZKHIP_OK;
}
static int tr_check_read(const zkhip_transcript* t, const void* p, size_t n, const char* who) {
  if (!t || (n && !p)) { set_error("%s: null pointer", who); return ZKHIP_EINVAL; }
  if (!t->reader) { set_error("%s: this transcript writes a proof", who); return ZKHIP_EINVAL; }
  if (n > TR_MAX || n * 32 > t->proof.size() - t->cursor) { set_error("%s: %zu elements asked for, %zu bytes of proof left", who, n, t->proof.size() - t->cursor); return ZKHIP_EINVAL; }
  return ZKHIP_OK;
}

}  // namespace zkhip

extern "C" {

zkhip_transcript* zkhip_transcript_new(int flag_layout) {
  if (flag_layout < 0 || flag_layout > 1) { set_error("transcript_new: flag_layout %d", flag_layout); return nullptr; }
  zkhip_transcript* t = new (std::nothrow) zkhip_transcript();
  if (!t) { set_error("transcript_new: out of memory"); return nullptr; }
  t->layout = flag_layout;
  t->st.init(64, (const uint8_t*)"Halo2-Transcript");
  return t;
}

zkhip_transcript* zkhip_transcript_new_reader(const uint8_t* proof, size_t len, int flag_layout) {
  if (len && !proof) { set_error("transcript_new_reader: null pointer"); return nullptr; }
  zkhip_transcript* t = zkhip_transcript_new(flag_layout);
  if (!t) return nullptr;
  t->reader = true;
  t->proof.assign(proof, proof + len);
  return t;
}

zkhip_transcript* zkhip_transcript_new_poseidon(int flag_layout) {
  if (flag_layout < 0 || flag_layout > 1) { set_error("transcript_new_poseidon: flag_layout %d", flag_layout); return nullptr; }
  zkhip_transcript* t = new (std::nothrow) zkhip_transcript();
  if (t) t->sponge = new (std::nothrow) zkhip::poseidon_sponge();
  if (!t || !t->sponge) { delete t; set_error("transcript_new_poseidon: out of memory"); return nullptr; }
  t->layout = flag_layout;
  t->poseidon = true;
  return t;
}

zkhip_transcript* zkhip_transcript_new_poseidon_reader(const uint8_t* proof, size_t len, int flag_layout) {
  if (len && !proof) { set_error("transcript_new_poseidon_reader: null pointer"); return nullptr; }
  zkhip_transcript* t = zkhip_transcript_new_poseidon(flag_layout);
  if (!t) return nullptr;
  t->reader = true;
  t->proof.assign(proof, proof + len);
  return t;
}

void zkhip_transcript_free(zkhip_transcript* t) {
  if (!t) return;
  delete t->sponge;
  if (t->pinned) { (void)hipHostFree(t->pinned); (void)hipGetLastError(); }
  delete t;
}

int zkhip_transcript_common_scalars(zkhip_transcript* t, const uint64_t* fr_mont, size_t n) {
  if (!t || (n && !fr_mont)) { set_error("transcript_common_scalars: null pointer"); return ZKHIP_EINVAL; }
  for (size_t i = 0; i < n; i++) {
    uint8_t repr[32];
    fr_mont_to_repr(fr_mont + i * 4, repr);
    tr_absorb_scalar(t, repr);
  }
  return ZKHIP_OK;
}

int zkhip_transcript_common_points(zkhip_transcript* t, const uint64_t* affine_mont, size_t n) {
  if (!t || (n && !affine_mont)) { set_error("transcript_common_points: null pointer"); return ZKHIP_EINVAL; }
  for (size_t i = 0; i < n; i++)
    if (bytes_zero((const uint8_t*)(affine_mont + i * 8), 64)) { set_error("transcript: cannot write points at infinity to the transcript (point %zu of %zu)", i, n); return ZKHIP_EINVAL; }
  for (size_t i = 0; i < n; i++) {
    uint8_t xy[64];
    fq_mont_to_repr(affine_mont + i * 8, xy);
    fq_mont_to_repr(affine_mont + i * 8 + 4, xy + 32);
    tr_absorb_point(t, xy);
  }
  return ZKHIP_OK;
}

int zkhip_transcript_squeeze(zkhip_transcript* t, uint64_t out_fr_mont[4]) {
  if (!t || !out_fr_mont) { set_error("transcript_squeeze: null pointer"); return ZKHIP_EINVAL; }
  if (t->poseidon) {
    const halo2::Fr c = t->sponge->squeeze();
    memcpy(out_fr_mont, c.l, 32);
    return ZKHIP_OK;
  }
  const uint8_t prefix = 0x00;
  t->st.update(&prefix, 1);
  uint8_t digest[64];
  t->st.digest(digest, 64);
  fr_reduce512(digest, out_fr_mont);
  return ZKHIP_OK;
}

int zkhip_transcript_write_scalars(zkhip_transcript* t, const uint64_t* fr_mont, size_t n) {
  int rc = tr_check_write(t, fr_mont, n, "transcript_write_scalars");
  if (rc != ZKHIP_OK) return rc;
  for (size_t i = 0; i < n; i++) {
    uint8_t repr[32];
    fr_mont_to_repr(fr_mont + i * 4, repr);
    tr_absorb_scalar(t, repr);
    t->proof.insert(t->proof.end(), repr, repr + 32);
  }
  return ZKHIP_OK;
}

int zkhip_transcript_write_points_device(zkhip_transcript* t, const void* d_points_xyz, size_t n, void* stream) {
  ZK_API_RANGE();
  int rc = tr_check_write(t, d_points_xyz, n, "transcript_write_points_device");
  if (rc != ZKHIP_OK) return rc;
  if ((uintptr_t)d_points_xyz & 15) { set_error("transcript_write_points_device: d_points_xyz must be 16-byte aligned"); return ZKHIP_EINVAL; }
  if (n == 0) return ZKHIP_OK;
  hipStream_t s = caller_stream(stream);
  scratch_pin P(s);                                        // g_mu is not held while the call waits for the stream and hashes
  if (P.rc != ZKHIP_OK) return P.rc;
  stream_drain drain(s);
  if ((rc = tr_write_points_core(t, P.sc, s, d_points_xyz, n)) != ZKHIP_OK) return rc;
  drain.done();
  return ZKHIP_OK;
}

int zkhip_transcript_write_scalars_device(zkhip_transcript* t, const void* d_fr, size_t n, void* stream) {
  ZK_API_RANGE();
  int rc = tr_check_write(t, d_fr, n, "transcript_write_scalars_device");
  if (rc != ZKHIP_OK) return rc;
  if ((uintptr_t)d_fr & 15) { set_error("transcript_write_scalars_device: d_fr must be 16-byte aligned"); return ZKHIP_EINVAL; }
  if (n == 0) return ZKHIP_OK;
  hipStream_t s = caller_stream(stream);
  scratch_pin P(s);                                        // g_mu is not held while the call waits for the stream and hashes
  if (P.rc != ZKHIP_OK) return P.rc;
  stream_drain drain(s);
  if ((rc = tr_write_scalars_core(t, P.sc, s, d_fr, n)) != ZKHIP_OK) return rc;
  drain.done();
  return ZKHIP_OK;
}

int zkhip_transcript_write_points(zkhip_transcript* t, const uint64_t* points_xyz, size_t n) {
  ZK_API_RANGE();
  int rc = tr_check_write(t, points_xyz, n, "transcript_write_points");
  if (rc != ZKHIP_OK) return rc;
  if (n == 0) return ZKHIP_OK;
  lane_hold H;                                             // drains its stream when the call leaves without finish()
  if (H.rc != ZKHIP_OK) return H.rc;
  if ((rc = H.sc->poly.reserve(n * 96)) != ZKHIP_OK) return rc;
  HIPCHK(hipMemcpyAsync(H.sc->poly.p, points_xyz, n * 96, hipMemcpyHostToDevice, H.s));
  if ((rc = tr_write_points_core(t, H.sc, H.s, H.sc->poly.p, n)) != ZKHIP_OK) return rc;
  return H.finish();
}

int zkhip_transcript_read_scalars(zkhip_transcript* t, size_t n, uint64_t* fr_mont) {
  int rc = tr_check_read(t, fr_mont, n, "transcript_read_scalars");
  if (rc != ZKHIP_OK) return rc;
  const uint8_t* src = t->proof.data() + t->cursor;
  for (size_t i = 0; i < n; i++)
    if (!fr_repr_to_mont(src + i * 32, fr_mont + i * 4)) { set_error("transcript: read_scalars: scalar %zu of %zu (proof byte %zu) is not below r", i, n, t->cursor + i * 32); return ZKHIP_EINVAL; }
  for (size_t i = 0; i < n; i++) tr_absorb_scalar(t, src + i * 32);
  t->cursor += n * 32;
  return ZKHIP_OK;
}

int zkhip_transcript_read_points_device(zkhip_transcript* t, size_t n, void* d_affine, void* stream) {
  ZK_API_RANGE();
  int rc = tr_check_read(t, d_affine, n, "transcript_read_points_device");
  if (rc != ZKHIP_OK) return rc;
  if ((uintptr_t)d_affine & 15) { set_error("transcript_read_points_device: d_affine must be 16-byte aligned"); return ZKHIP_EINVAL; }
  if (n == 0) return ZKHIP_OK;
  hipStream_t s = caller_stream(stream);
  scratch_pin P(s);                                        // g_mu is not held while the call waits for the stream and hashes
  if (P.rc != ZKHIP_OK) return P.rc;
  stream_drain drain(s);
  if ((rc = tr_read_points_core(t, P.sc, s, n, d_affine, nullptr)) != ZKHIP_OK) return rc;
  drain.done();
  return ZKHIP_OK;
}

int zkhip_transcript_read_points(zkhip_transcript* t, size_t n, uint64_t* affine_mont) {
  ZK_API_RANGE();
  int rc = tr_check_read(t, affine_mont, n, "transcript_read_points");
  if (rc != ZKHIP_OK) return rc;
  if (n == 0) return ZKHIP_OK;
  lane_hold H;
  if (H.rc != ZKHIP_OK) return H.rc;
  if ((rc = H.sc->bases.reserve(n * 64)) != ZKHIP_OK) return rc;
  if ((rc = tr_read_points_core(t, H.sc, H.s, n, H.sc->bases.p, affine_mont)) != ZKHIP_OK) return rc;
  return H.finish();
}

int zkhip_transcript_proof(const zkhip_transcript* t, uint8_t* buf, size_t cap, size_t* len) {
  if (!t || !len) { set_error("transcript_proof: null pointer"); return ZKHIP_EINVAL; }
  *len = t->proof.size();
  if (!buf) return ZKHIP_OK;
  if (cap < t->proof.size()) { set_error("transcript_proof: %zu bytes of room, %zu needed", cap, t->proof.size()); return ZKHIP_EINVAL; }
  if (!t->proof.empty()) memcpy(buf, t->proof.data(), t->proof.size());
  return ZKHIP_OK;
}

int zkhip_test_reduce512(const uint8_t in64[64], uint64_t out_fr_mont[4]) {
  if (!in64 || !out_fr_mont) { set_error("test_reduce512: null pointer"); return ZKHIP_EINVAL; }
  fr_reduce512(in64, out_fr_mont);
  return ZKHIP_OK;
}

uint32_t zkhip_test_transcript_chunk(size_t n) { return transcript_chunk(n); }

}  // extern "C"
