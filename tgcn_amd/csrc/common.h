// common.h -- error reporting, launch timing, tuning switches and small host helpers shared by every section
// Part of the single translation unit tgcn_hip.hip (included once, inside its anonymous namespace).
#pragma once


thread_local char g_err[512] = "";

#define TGCN_FAIL(code, ...)                    \
  do {                                          \
    snprintf(g_err, sizeof(g_err), __VA_ARGS__); \
    return (code);                              \
  } while (0)

#define TGCN_CHECK_LAUNCH(what)                                                         \
  do {                                                                                  \
    hipError_t e_ = hipGetLastError();                                                  \
    if (e_ != hipSuccess) TGCN_FAIL(TGCN_ERR_LAUNCH, "%s: %s", what, hipGetErrorString(e_)); \
  } while (0)

constexpr int kBlock = 256;

// ---- optional launch timing (bench / tests): hipEvent pairs recorded around launches on their own stream.
// State of the CALLING THREAD (round 6: the ABI holds no process-global mutable state): a thread that asked for a
// record gets the launches IT issues; the replicas' threads of an nn.DataParallel process neither see nor disturb it.
struct ProfRec { hipEvent_t a, b; int kind; };
thread_local std::vector<ProfRec> g_prof;
thread_local int g_prof_cap = 0;

struct ProfScope {
  hipEvent_t b = nullptr;
  hipStream_t st;
  ProfScope(int kind, hipStream_t s) : st(s) {
    if (g_prof_cap <= 0) return;
    if ((int)g_prof.size() >= g_prof_cap) return;
    ProfRec r;
    if (hipEventCreate(&r.a) != hipSuccess || hipEventCreate(&r.b) != hipSuccess) return;
    r.kind = kind;
    (void)hipEventRecord(r.a, st);
    b = r.b;
    g_prof.push_back(r);
  }
  ~ProfScope() { if (b) (void)hipEventRecord(b, st); }
};

// Kernels that take more than 64 KB of dynamic LDS.  The attribute belongs to the calling thread's current device
// (nn.DataParallel drives several devices from one process), so it is kept per (device, kernel): set on the first request and raised
// when a later launch of the same kernel asks for more (series_gemm_launch and hop_kernel's pad pass the launch's own size).
inline void allow_large_lds(const void* fn, int bytes) {
  static std::mutex mu;
  static std::map<std::pair<int, const void*>, int> largest;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return;
  std::lock_guard<std::mutex> lk(mu);
  int& have = largest[std::make_pair(dev, fn)];
  if (bytes > have) {
    (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);   // a refusal surfaces as a launch error
    have = bytes;
  }
}

// ---- run-time values as compile-time constants: how a launcher picks a kernel's template instantiation.  f is a generic lambda; its
// arguments carry the values in their types (std::true_type / std::false_type, std::integral_constant<int, V>) and convert back to them
// in a constant expression, template arguments included: with_flags([&](auto vec) { launch_kernel(some_kernel<vec>, ...); }, is_vec).
// A launcher that builds only some combinations guards the body with `if constexpr (..._form_built(flags))`: the others are never instantiated.
template <class F>
inline void with_flags(F&& f) { f(); }
template <class F, class... B>
inline void with_flags(F&& f, bool b, B... rest) {
  if (b) with_flags([&](auto... c) { f(std::true_type{}, c...); }, rest...);
  else with_flags([&](auto... c) { f(std::false_type{}, c...); }, rest...);
}
// v out of the list Vs; a value that is not in it takes the last
template <int V, int... Vs, class F>
inline void with_one_of(int v, F&& f) {
  if constexpr (sizeof...(Vs) == 0) f(std::integral_constant<int, V>{});
  else if (v == V) f(std::integral_constant<int, V>{});
  else with_one_of<Vs...>(v, f);
}

// Dynamic LDS of a launch and what its kernel is opted in to first (allow_large_lds): the launch's own bytes where they exceed the 64 KB every
// kernel may take, or the family's largest where a launcher names it.
struct DynLds {
  size_t bytes;
  int optin;
  DynLds(size_t b) : bytes(b), optin(b > 64 * 1024 ? (int)b : 0) {}
  DynLds(size_t b, int most) : bytes(b), optin(most) {}
};
template <class... P, class... A>
inline void launch_kernel(void (*kernel)(P...), dim3 grid, dim3 block, DynLds lds, hipStream_t st, const A&... args) {
  if (lds.optin) allow_large_lds((const void*)kernel, lds.optin);
  hipLaunchKernelGGL(kernel, grid, block, lds.bytes, st, args...);
}
// A grid of nblk x gy workgroups in launches of at most `part` along x (a launch holds fewer than 2^32 threads along x, tgcn_hip.hip
// kSeriesGridPart); each part is told its first workgroup in p.blk0, the kernel's first argument.
template <class... P, class Params, class... A>
inline void launch_kernel_parts(void (*kernel)(P...), int64_t nblk, int64_t part, unsigned gy, dim3 block, DynLds lds, hipStream_t st, Params& p,
                                const A&... extra) {
  if (lds.optin) allow_large_lds((const void*)kernel, lds.optin);
  for (int64_t b0 = 0; b0 < nblk; b0 += part) {
    p.blk0 = (decltype(p.blk0))b0;
    hipLaunchKernelGGL(kernel, dim3((unsigned)std::min<int64_t>(part, nblk - b0), gy), block, lds.bytes, st, p, extra...);
  }
}

// Compute units of the calling thread's current device (256 on MI355X), read once per device: round sizes of one-workgroup-per-CU
// kernels follow from it instead of a literal.
// Dynamic LDS a workgroup of the calling thread's current device can opt in to (163,840 B on gfx950; 65,536 on gfx942), read once per device:
// kernels that keep a whole weight resident (project_x3_stream_kernel: up to 150 KB) are only chosen where it fits, the tiled forms otherwise.
inline int lds_optin_limit() {
  static std::atomic<int> cached[16];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return 64 * 1024;
  int v = cached[dev].load(std::memory_order_relaxed);
  if (v > 0) return v;
  if (hipDeviceGetAttribute(&v, hipDeviceAttributeSharedMemPerBlockOptin, dev) != hipSuccess || v <= 0) {
    (void)hipGetLastError();
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess || v <= 0) v = 64 * 1024;
  }
  cached[dev].store(v, std::memory_order_relaxed);
  return v;
}

inline int cu_count() {
  static std::atomic<int> cached[16];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return 256;
  int v = cached[dev].load(std::memory_order_relaxed);
  if (v > 0) return v;
  if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = 256;
  cached[dev].store(v, std::memory_order_relaxed);
  return v;
}

// ---- developer switches (tgcn_set_tuning): state of the CALLING THREAD, like the launch timing above.  A switch set by a test or a tool
// selects another kernel for the same arithmetic in the launches that thread issues afterwards; other threads (DataParallel replicas,
// the autograd engine's workers) keep the defaults, which are what ships.
struct TuneInt {
  int v;
  int load() const { return v; }
  void store(int x) { v = x; }
};
thread_local TuneInt g_hop_variant{0};
thread_local TuneInt g_hop_remap{1};        // hop_kernel: row blocks in XCD-contiguous ranges (1) or round robin over the XCDs (0)
thread_local TuneInt g_hop_seg_remap{0};    // hop_kernel: segment blocks in XCD-contiguous ranges (1) or round robin over the XCDs (0)
thread_local TuneInt g_hop_mix{0};          // hop_kernel: row blocks dealt evenly among the segment blocks (1) or all in front (0)
thread_local TuneInt g_hop_stream{1};       // hop_kernel: non-temporal entries / stores / partial rows when the output exceeds the Infinity Cache (0: never)
thread_local TuneInt g_hop_lds_pad{0};      // hop_kernel: bytes of unused dynamic LDS per workgroup (occupancy limiter, developer A/B)
thread_local TuneInt g_sched_hub_min{512};     // tgcn_sched_build, 16-lane schedules: rows of more entries are cut into wave segments (0: never) ...
thread_local TuneInt g_sched_hub_seg{64};      // ... of this many entries ...
thread_local TuneInt g_sched_hub_gate_mb{256};  // ... where the plain schedule's partial rows take more than this many MiB (tgcn_amd/graph.py: HUB_MIN, HUB_SEG, HUB_GATE_BYTES)
thread_local TuneInt g_proj_variant{0};     // 1: force the streaming-W kernel
thread_local TuneInt g_x3_form{2};          // bf16x3 projection, aligned operands, >= 96 output columns: 2 = A fragments from registers (+20 %), 1 = both operands through LDS
thread_local TuneInt g_x3_tail{1};          // project_x3v2_kernel: rows of a thinly filled last round as 128-row tiles (0: 256-row tiles throughout)
thread_local TuneInt g_small_narrow{1};     // C <= 4 inputs of the one-launch path: input-side recursion (0: output-side kernel)
thread_local TuneInt g_small_dense{2};      // small dense operands: 2 bf16x3 matrix pipe, 1 fp32 matrix pipe, 0 vector-ALU kernels only
thread_local TuneInt g_x3_stream_cap{0};    // project_x3_claim_kernel: workgroups per launch (0: one per two CUs, docs/EXPERIMENTS.md A.7)
thread_local TuneInt g_overlap{1};          // compacted layer: projections on the side stream beside the hops (0: everything on the caller's stream)
thread_local TuneInt g_overlap_group{3};    // ... time steps per group: a group's kept-row projection runs beside the next group's hops
thread_local TuneInt g_overlap_min_mb{256}; // ... only when one time step's hop tensor is larger than this many MB (the Infinity Cache)

// ---- the library's own side stream (compacted layer: projections beside the hops).  One lowest-priority, non-blocking
// stream and a small pool of events per CALLING THREAD and device, created on first use and kept for the life of the process (a thread's
// exit may come after the runtime's: nothing is destroyed).  Events are handed out round robin: hipStreamWaitEvent takes the record that
// is current when it is called, so an event may be recorded again as soon as its wait has been issued.
struct SideStream {
  hipStream_t st = nullptr;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  int next = 0;
  hipEvent_t event() { hipEvent_t e = ev[next]; next = (next + 1) & 3; return e; }
};
thread_local std::map<int, SideStream>* g_side = nullptr;
thread_local int64_t g_side_launches = 0;      // kernels the calling thread has put on its side streams (tgcn_side_stream_launches)

inline SideStream* side_stream() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  if (!g_side) g_side = new std::map<int, SideStream>();
  SideStream& s = (*g_side)[dev];
  if (s.st) return &s;
  int least = 0, greatest = 0;
  if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) { (void)hipGetLastError(); least = 0; }
  // events first, the stream last: whatever a failed attempt did create is kept in `s` and reused by the next one
  for (auto& e : s.ev)
    if (!e && hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); e = nullptr; return nullptr; }
  if (hipStreamCreateWithPriority(&s.st, hipStreamNonBlocking, least) != hipSuccess) { (void)hipGetLastError(); s.st = nullptr; return nullptr; }
  return &s;
}

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Device of a caller's data pointer against the calling thread's current device.  The stream a caller hands in belongs to its current
// device, and every launch goes there: a module moved to cuda:1 and called while cuda:0 is current would run on the wrong GPU (the
// reference's torch ops follow the TENSOR's device, tgcn/nn/gcn.py:141,147; SURVEY.md 8b "honour ... the device of the pointers").
// One hipPointerGetAttributes per layer / hop call; skipped while the stream is being captured into a hipGraph (the capture was started
// on that device by construction).
inline int check_pointer_device(const void* p, hipStream_t st, const char* who) {
  if (!p) return TGCN_OK;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cs) != hipSuccess) { (void)hipGetLastError(); return TGCN_OK; }
  if (cs != hipStreamCaptureStatusNone) return TGCN_OK;
  int cur = -1;
  if (hipGetDevice(&cur) != hipSuccess) return TGCN_OK;
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return TGCN_OK; }    // not a pointer the runtime knows: nothing to say
  if (at.type == hipMemoryTypeDevice && at.device != cur)
    TGCN_FAIL(TGCN_ERR_INVALID, "%s: the data is on device %d but the calling thread's current device is %d -- make the tensor's device current "
                                "(hipSetDevice / torch.cuda.device) and pass that device's stream", who, at.device, cur);
  return TGCN_OK;
}
