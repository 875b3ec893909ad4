// Library-wide state of libstarkperp: the selected device, the HBM-resident window tables and
// growable scratch.  One context per process (one process per GPU).
#pragma once
#include <hip/hip_runtime.h>
#include <condition_variable>
#include <cstring>
#include <functional>
#include <initializer_list>
#include <mutex>
#include <utility>
#include <string>

#include "../../include/starkperp.h"
#include "curve.hpp"
#include "u256.hpp"

namespace sp {

// 64-byte table entry: affine point, Montgomery form, canonical 256-bit packing.
struct alignas(64) aff_packed {
  u256 x, y;
};

// Window plan of the Pedersen tables over the 504-bit string  x (252 bits) || y (252 bits).
// Window 0 is unsigned: `bits[0]` bits, 2^bits[0] entries.  Every other window is SIGNED: it covers
// log2e + 1 bits with 2^log2e entries - the top bit of the window is the sign of the whole entry
// (see context.hip).  Windows may straddle the x | y boundary.
constexpr int PED_MAX_WINDOWS = 128;
struct PedPlan {
  int nwin = 0;
  int log2e = 0;                       // entries per signed window = 2^log2e  (what sp_window_bits reports)
  uint16_t start[PED_MAX_WINDOWS];     // first bit of window g in the 504-bit string
  uint8_t bits[PED_MAX_WINDOWS];       // bits the window consumes
  uint64_t base[PED_MAX_WINDOWS];      // index of the window's first entry in the table
  uint64_t entries = 0;                // total
};

struct DeviceBuffer {
  void* ptr = nullptr;
  size_t bytes = 0;
  // Grow-only; contents are not preserved.
  hipError_t reserve(size_t need) {
    if (need <= bytes) return hipSuccess;
    if (ptr) (void)hipFree(ptr);
    ptr = nullptr;
    bytes = 0;
    size_t want = need + need / 4;
    hipError_t e = hipMalloc(&ptr, want);
    if (e == hipSuccess) bytes = want;
    return e;
  }
  void release() {
    if (ptr) (void)hipFree(ptr);
    ptr = nullptr;
    bytes = 0;
  }
};

// Page-locked host memory for staging SMALL host-pointer batches (round 6).  A hipMemcpyAsync from pageable memory
// makes the runtime pin / unpin the caller's pages around every copy; when two host threads of one call do that at
// the same time - sp_order_batch's tree update and its verifier thread - one of them was seen to stall for 6 - 11 ms
// (profiles/r06_c3_host_timeline.txt).  Staged copies (memcpy into this buffer, then a truly asynchronous DMA) have no
// such path.  Batches above PINNED_STAGE_MAX keep the direct copy: they are throughput-bound, and page-locking hundreds
// of megabytes per lane would cost more than it saves.
constexpr size_t PINNED_STAGE_MAX = (size_t)4 << 20;
struct PinnedBuffer {
  void* ptr = nullptr;
  size_t bytes = 0;
  hipError_t reserve(size_t need) {  // grow-only; contents are not preserved
    if (need <= bytes) return hipSuccess;
    release();
    size_t want = need + need / 4;
    hipError_t e = hipHostMalloc(&ptr, want, hipHostMallocDefault);
    if (e == hipSuccess) bytes = want;
    return e;
  }
  void release() {  // wiped first: a signer's private keys and nonces may have crossed it (StagedTrip::secret)
    if (ptr) explicit_bzero(ptr, bytes);
    if (ptr) (void)hipHostFree(ptr);
    ptr = nullptr;
    bytes = 0;
  }
};

// One host array of a staged round trip.  A null `ptr` keeps its `bytes` in the layout and is copied in neither branch:
// an output the caller did not ask for, or padding between two device arrays.
struct Piece {
  void* ptr;
  size_t bytes;
  Piece(const void* p, size_t b) : ptr(const_cast<void*>(p)), bytes(b) {}
};
// The round trip of a host-pointer call whose inputs are adjacent on the device and whose outputs are too.  The
// constructor makes the PinnedBuffer decision for `bytes` (inputs + outputs) - the only place that does:
//   stage != nullptr   STAGED: the pieces share one page-locked block, inputs first, and cross in one copy each way;
//   stage == nullptr   DIRECT: one copy per piece, from / into the caller's arrays (a batch above PINNED_STAGE_MAX, or
//                      a page-locked allocation that failed - its error is cleared here).
// up() before the kernels, down() behind them, finish() after the caller's own wait on the stream.  A call whose copies
// have another shape (tree_enqueue, the large page of sp_tree_scan) reads `stage` and copies for itself.
// secret(at, bytes) before up() marks a range of the inputs as private keys or nonces: the block's copy of it is zeroed
// by finish() and, on a path that never gets there, by the destructor (include/starkperp.h "threat model": at rest).
struct StagedTrip {
  char* stage = nullptr;
  hipStream_t st;
  size_t up_bytes = 0;  // where the outputs start in the block
  size_t secret_at = 0, secret_bytes = 0;
  static bool fits(size_t bytes) { return bytes <= PINNED_STAGE_MAX; }
  StagedTrip(PinnedBuffer& buf, size_t bytes, hipStream_t stream) : st(stream) {
    if (fits(bytes) && buf.reserve(bytes) == hipSuccess) stage = (char*)buf.ptr;
    else (void)hipGetLastError();
  }
  ~StagedTrip() { wipe(); }
  StagedTrip(const StagedTrip&) = delete;
  StagedTrip& operator=(const StagedTrip&) = delete;
  void secret(size_t at, size_t bytes) { secret_at = at; secret_bytes = bytes; }
  void wipe() {  // explicit_bzero: a store the compiler may not drop
    if (stage && secret_bytes) explicit_bzero(stage + secret_at, secret_bytes);
    secret_bytes = 0;
  }
  // the host pieces -> dev, one behind the other
  hipError_t up(void* dev, std::initializer_list<Piece> pieces) {
    size_t at = 0;
    for (const Piece& p : pieces) {
      if (p.ptr && stage) std::memcpy(stage + at, p.ptr, p.bytes);
      if (p.ptr && !stage) {
        const hipError_t e = hipMemcpyAsync((char*)dev + at, p.ptr, p.bytes, hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return e;
      }
      at += p.bytes;
    }
    up_bytes = at;
    return stage ? hipMemcpyAsync(dev, stage, at, hipMemcpyHostToDevice, st) : hipSuccess;
  }
  // dev, one piece behind the other -> the block (staged) or the host pieces (direct); enqueued only
  hipError_t down(const void* dev, std::initializer_list<Piece> pieces) {
    size_t at = 0;
    for (const Piece& p : pieces) {
      if (p.ptr && !stage) {
        const hipError_t e = hipMemcpyAsync(p.ptr, (const char*)dev + at, p.bytes, hipMemcpyDeviceToHost, st);
        if (e != hipSuccess) return e;
      }
      at += p.bytes;
    }
    return stage ? hipMemcpyAsync(stage + up_bytes, dev, at, hipMemcpyDeviceToHost, st) : hipSuccess;
  }
  // after the wait: the block -> the host pieces (direct: they are there already); the secret inputs leave the block
  void finish(std::initializer_list<Piece> pieces) {
    size_t at = up_bytes;
    for (const Piece& p : pieces) {
      if (p.ptr && stage) std::memcpy(p.ptr, stage + at, p.bytes);
      at += p.bytes;
    }
    wipe();
  }
};

// Device memory that grows without a device-wide wait: hipFree synchronises the whole device (in sp_order_batch it
// stalled the verification running beside a tree update), so the allocation a growth replaces is RETIRED, not freed -
// work already on the stream may still read it, and grow() hands it back for the caller's own copy or rehash out of
// it.  It is freed at the next growth, behind a wait for the one stream, or by release().  Sizing is the caller's.
template <class T>
struct RetiringBuffer {
  T* ptr = nullptr;
  T* retired = nullptr;
  size_t bytes = 0;
  hipError_t grow(size_t want, hipStream_t st, T** old = nullptr) {
    if (retired) {  // the allocation before the last one: only work older than the last growth can still read it
      const hipError_t e = hipStreamSynchronize(st);
      if (e != hipSuccess) return e;
      (void)hipFree(retired);
      retired = nullptr;
    }
    T* fresh = nullptr;
    const hipError_t e = hipMalloc(&fresh, want);
    if (e != hipSuccess) return e;
    retired = ptr;
    ptr = fresh;
    bytes = want;
    if (old) *old = retired;
    return hipSuccess;
  }
  void release() {
    if (ptr) (void)hipFree(ptr);
    if (retired) (void)hipFree(retired);
    ptr = retired = nullptr;
    bytes = 0;
  }
};

// One context per device the process drives (sp_init: one; sp_init_devices: several).  Context 0 is the
// PRIMARY: the stateful machinery - persistent trees, the ECDSA key cache, the prover's twiddle tables and
// witness scratch - lives on its device only.  The stateless batches (hash, ladder verification, signing,
// public keys, tree / forest rebuilds, row commitments) run on any context: a host-pointer call takes the
// context of the host lane it was given, a _dev call the context of the device its pointers live on.
constexpr int SP_MAX_CONTEXTS = 16;
std::recursive_mutex& global_mu();
struct Context {
  bool ready = false;
  int device = -1;
  int wbits = 16;        // EC_GEN table: window width
  int nwin = 16;         // EC_GEN table: windows per 252-bit scalar = ceil(252 / wbits)
  aff_packed* ped = nullptr;   // Pedersen window tables, laid out by `plan`
  aff_packed* gen = nullptr;   // [nwin][1 << wbits]     fixed-base EC_GEN
  // STARKPERP_SIGN_MASKED=1: a second EC_GEN table of 63 unsigned 4-bit windows (63 x 16 entries = 63 KiB) for the
  // signers and the key derivation: every window reads all 16 of its entries and keeps one by a mask, so no address
  // depends on the nonce or the private key (ecdsa.hip gen_mul_masked; include/starkperp.h "threat model")
  aff_packed* gen_masked = nullptr;
  // the fixed-base table the SECRET-scalar kernels are handed: wbits < 0 selects the masked walk
  const aff_packed* secret_gen() const { return gen_masked ? gen_masked : gen; }
  int secret_wbits() const { return gen_masked ? -4 : wbits; }
  int secret_nwin() const { return gen_masked ? 63 : nwin; }
  PedPlan plan;                // host copy
  PedPlan* d_plan = nullptr;   // device copy the kernels read (uniform loads)
  size_t table_bytes = 0;
  uint64_t host_calls = 0;     // host-lane calls served (sp_context_info)
  // Recursive: an entry point that holds it may call a _dev entry point, which takes it again.  ONE lock for all
  // contexts: it also guards the per-stream scratch maps, which are shared; it is held while work is
  // enqueued, never while the device runs a stateless batch.
  std::recursive_mutex& mu = global_mu();
};
using ctx_lock = std::lock_guard<std::recursive_mutex>;

Context& ctx();               // the context selected on this host thread (the primary unless a scope below says otherwise)
Context& ctx_at(int index);
int ctx_count();
int ctx_current();
void ctx_select(int index);
// Key of the per-stream scratch maps: the null stream exists once per device.
using StreamKey = std::pair<int, hipStream_t>;
inline StreamKey stream_key(hipStream_t st) { return StreamKey(ctx_current(), st); }

// Selects, for the duration of a _dev entry point, the context whose device owns `device_ptr`.  With one
// context (the common case: one process per GPU) it does nothing.
struct CtxByPointer {
  int previous;
  explicit CtxByPointer(const void* device_ptr);
  ~CtxByPointer() { ctx_select(previous); }
  CtxByPointer(const CtxByPointer&) = delete;
  CtxByPointer& operator=(const CtxByPointer&) = delete;
};

// Host lanes: the host-pointer entry points that carry no shared state (hash / verify / sign / public-key
// batches) each take one of HOST_LANES lanes - a non-blocking stream with its own staging buffer - so that
// calls from different host threads overlap on the device instead of queueing behind one lock (the scalar
// API of the reference is a stream of one-item calls: 0.1 - 0.4 ms of latency each, almost all of it idle
// chip).  The context lock is then held only while a kernel is enqueued.  A caller blocks while every lane is
// taken.  Lane i belongs to context i mod ctx_count(), and lanes are handed out round-robin: concurrent
// callers spread over the devices of sp_init_devices.
constexpr int HOST_LANES = 16;
struct HostLane {
  hipStream_t stream = nullptr;
  int stream_ctx = -1;          // the context the stream was created for
  DeviceBuffer io;              // grow-only until sp_shutdown: one huge batch parks its buffer on its lane
  PinnedBuffer hio;             // host-side staging of small batches (see PinnedBuffer)
  bool busy = false;
};
HostLane* lane_acquire(int* ctx_index, int want_ctx);  // want_ctx < 0: any context, round-robin
void lane_release(HostLane* lane);
void lane_drain(HostLane* lane);  // waits for whatever is still queued on the lane's stream
int lane_stream(HostLane* lane);  // creates the lane's stream on the current device if needed; SP_OK or SP_ERR_HIP
void release_host_lanes();        // sp_shutdown
// ecdsa.hip: keyed verification of a host batch; `before_lock` runs once, after the lock-free part and before the
// library lock is taken (also when there is nothing to verify).
int verify_batch_keyed_gated(const uint64_t* z, const uint64_t* r, const uint64_t* s, const uint64_t* qx,
                             const uint64_t* qy, uint8_t* result, size_t n, const std::function<void()>& before_lock);
// Usage in an entry point:  LaneScope ls;  SP_REQUIRE_READY();  if (ls.open() != SP_OK) return SP_ERR_HIP;
// A large host batch on several contexts: `fn(offset, count)` runs once per context on its own host thread, each
// bound to its context (so the LaneScope inside takes a lane of that context), over contiguous slices of the n
// items; returns the first non-zero code.  Used by the stateless host-pointer batches when ctx_count() > 1.
int shard_over_contexts(size_t n, const std::function<int(size_t, size_t)>& fn);
int shard_context();  // the context this host thread was bound to by shard_over_contexts, or -1
constexpr size_t SHARD_MIN_ITEMS = 16384;  // below this one device is faster than the host threads are to start

struct LaneScope {
  HostLane* lane;
  int previous_ctx;
  LaneScope() : previous_ctx(ctx_current()) {
    int index = 0;
    lane = lane_acquire(&index, shard_context());
    ctx_select(index);
  }
  explicit LaneScope(int want_ctx) : previous_ctx(ctx_current()) {  // a lane of one particular context
    int index = 0;
    lane = lane_acquire(&index, want_ctx);
    ctx_select(index);
  }
  int open() { return lane_stream(lane); }
  ~LaneScope() {
    // An entry point that leaves early (a failed HIP call) may still have copies into the CALLER's buffers
    // or kernels on the lane's staging buffer in flight: drain the stream before the lane - and, on the
    // caller's side, the buffers - can be reused.  After a normal return the stream is idle and this is free.
    lane_drain(lane);
    lane_release(lane);
    ctx_select(previous_ctx);
  }
  LaneScope(const LaneScope&) = delete;
  LaneScope& operator=(const LaneScope&) = delete;
};

void set_error(const std::string& s);
// call `who` refuses an argument: "<who>: <bad>" for sp_last_error
inline int refuse(const char* who, const char* bad) {
  set_error(std::string(who) + ": " + bad);
  return SP_ERR_BAD_ARGUMENT;
}
// stark.hip: 1 / (x^n - 1) at the four residues i mod 4 of the coset, or SP_ERR_BAD_ARGUMENT for a shift it vanishes on
int air_zinv(const char* who, const uint64_t* shift_host, unsigned log_n, bool times_r2, fe zinv[4]);
// the shift rule of the composition calls: below p, not 0, shift^(4n) != 1 (air_zinv names the call and says "shift")
inline int check_shift(const char* who, const uint64_t* shift_host, unsigned log_n) {
  u256 sh;
  std::memcpy(sh.w, shift_host, 32);
  if (!u256_lt(sh, U256_P)) return refuse(who, "bad shift (not below p)");
  fe unused[4];
  return air_zinv(who, shift_host, log_n, false, unused);
}

// Host-side timeline of ONE traced API call (diagnostics, STARKPERP_TIMELINE=1; tools/c3_probe.py): marks from any
// thread of the call - the caller's and sp_order_batch's verifier - printed to stderr as one line when the call
// ends.  With the variable unset tl_mark is one relaxed load and a branch.
struct HostTimeline;
void tl_mark(const char* what);
struct TimelineScope {  // opens the timeline for the duration of a call (no-op unless STARKPERP_TIMELINE=1)
  HostTimeline* mine = nullptr;
  explicit TimelineScope(const char* call);
  ~TimelineScope();
  TimelineScope(const TimelineScope&) = delete;
  TimelineScope& operator=(const TimelineScope&) = delete;
};
int hip_fail(hipError_t e, const char* what);
// pedersen.hip: the event pair of sp_profile_begin/_end around one launch of another file; call both under the
// library lock, _end only after _begin returned true
bool profile_launch_begin(hipStream_t st);
void profile_launch_end(hipStream_t st, size_t units);

// whether two caller arrays share a byte (an output of a batch call may not overlap an input)
inline bool overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  const char *p = (const char*)a, *q = (const char*)b;
  return p < q + b_bytes && q < p + a_bytes;
}

#define SP_HIP(call)                                   \
  do {                                                 \
    hipError_t e__ = (call);                           \
    if (e__ != hipSuccess) return hip_fail(e__, #call); \
  } while (0)

// HIP's current device is per host thread: a thread other than the one that called sp_init would
// otherwise launch on device 0.  Binds the library's device for the duration of an entry point and
// puts the caller's own choice back afterwards.
struct DeviceScope {
  int previous = -1;
  bool switched = false;
  explicit DeviceScope(int device) {
    if (hipGetDevice(&previous) == hipSuccess && previous != device) switched = hipSetDevice(device) == hipSuccess;
  }
  ~DeviceScope() {
    if (switched) (void)hipSetDevice(previous);
  }
  DeviceScope(const DeviceScope&) = delete;
  DeviceScope& operator=(const DeviceScope&) = delete;
};

#define SP_REQUIRE_READY()                                                        \
  if (!ctx().ready) {                                                             \
    set_error("libstarkperp is not initialised (sp_init failed or not called; "   \
              "there is no CPU fallback)");                                       \
    return SP_ERR_NOT_INITIALISED;                                                \
  }                                                                               \
  sp::DeviceScope sp_device_scope__(ctx().device)

// ---- device helpers shared by the kernels ----
__device__ __forceinline__ u256 ld_u256(const uint64_t* p) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
  uint4 a = q[0], b = q[1];
  u256 r;
  r.w[0] = a.x; r.w[1] = a.y; r.w[2] = a.z; r.w[3] = a.w;
  r.w[4] = b.x; r.w[5] = b.y; r.w[6] = b.z; r.w[7] = b.w;
  return r;
}
__device__ __forceinline__ void st_u256(uint64_t* p, const u256& v) {
  uint4* q = reinterpret_cast<uint4*>(p);
  q[0] = make_uint4(v.w[0], v.w[1], v.w[2], v.w[3]);
  q[1] = make_uint4(v.w[4], v.w[5], v.w[6], v.w[7]);
}
__device__ __forceinline__ aff ld_aff(const aff_packed* e) {
  const uint4* q = reinterpret_cast<const uint4*>(e);
  uint4 a = q[0], b = q[1], c = q[2], d = q[3];
  u256 x, y;
  x.w[0] = a.x; x.w[1] = a.y; x.w[2] = a.z; x.w[3] = a.w;
  x.w[4] = b.x; x.w[5] = b.y; x.w[6] = b.z; x.w[7] = b.w;
  y.w[0] = c.x; y.w[1] = c.y; y.w[2] = c.z; y.w[3] = c.w;
  y.w[4] = d.x; y.w[5] = d.y; y.w[6] = d.z; y.w[7] = d.w;
  aff r;
  r.x = fe_unpack(x);
  r.y = fe_unpack(y);
  return r;
}
// u256_lt, u256_is_zero and the bounds U256_P / U256_N / U256_2P251: u256.hpp

// w-bit window number `win` of a 256-bit little-endian integer
__device__ __forceinline__ uint32_t window_of(const u256& a, int win, int wbits) {
  const int bit = win * wbits, wi = bit >> 5, sh = bit & 31;
  uint64_t two = (uint64_t)a.w[wi] | ((uint64_t)(wi + 1 < 8 ? a.w[wi + 1] : 0u) << 32);
  return (uint32_t)(two >> sh) & ((1u << wbits) - 1u);
}

}  // namespace sp
