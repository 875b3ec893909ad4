// Batch square roots mod p and x-only Stark keys: sqrt_mod / is_quad_residue (math_utils.py:36-47), get_y_coordinate
// (signature.py:84-96) and is_valid_stark_key (signature.py:204-214), one item per lane.
//
// The arithmetic is csrc/fp29.hpp fe_sqrt (a fixed 2 338 field operations per root, whatever the input) and
// csrc/stark_keys.hpp stark_key_item, which the host tests run under g++ as well.  A launch is latency-bound: one lane
// walks ~2 300 dependent squarings, so up to 2^16 items (one wave per SIMD) take the time of one item's chain; the 25
// table entries and 24 hash bytes an item reads come from a 204 KiB table that stays in L2.
#include <memory>

#include "context.hpp"
#include "stark_keys.hpp"

namespace sp {

constexpr int KEYS_TPB = 128;

template <bool KEY, bool WANT_ROOT>
__global__ void __launch_bounds__(KEYS_TPB)
stark_keys_kernel(const uint64_t* __restrict__ in, uint64_t* __restrict__ out, uint8_t* __restrict__ status, size_t n,
                  const sqrt_tables* __restrict__ tab) {
  // Lanes past the end redo the last item instead of idling (identical reads, identical writes), as
  // ecdsa_verify_kernel does: a wave with few active lanes runs VALU code several times slower on this chip.
  size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) e = n - 1;
  u256 res;
  const uint8_t code = stark_key_item<KEY, WANT_ROOT>(ld_u256(in + 4 * e), tab, res);
  status[e] = code;
  if (WANT_ROOT && code == SP_SQRT_OK) st_u256(out + 4 * e, res);
}

// The tables: built once per process on the host (fp29.hpp sqrt_tables_build, from 3 and m), uploaded per context by
// the first root call that runs there.  All under the library lock.
static std::unique_ptr<sqrt_tables> g_sqrt_host;
static sqrt_tables* g_sqrt_dev[SP_MAX_CONTEXTS] = {};

static int sqrt_tables_for_context(const sqrt_tables** tab) {
  const int at = ctx_current();
  if (!g_sqrt_dev[at]) {
    if (!g_sqrt_host) {
      std::unique_ptr<sqrt_tables> fresh(new sqrt_tables);
      if (!sqrt_tables_build(*fresh)) {
        set_error("square-root tables: 3^m does not generate the 2^192 subgroup, or no hash multiplier was found");
        return SP_ERR_TABLE_BUILD;
      }
      g_sqrt_host = std::move(fresh);
    }
    sqrt_tables* dev = nullptr;
    SP_HIP(hipMalloc(&dev, sizeof(sqrt_tables)));
    const hipError_t e = hipMemcpy(dev, g_sqrt_host.get(), sizeof(sqrt_tables), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      (void)hipFree(dev);
      return hip_fail(e, "hipMemcpy (square-root tables)");
    }
    g_sqrt_dev[at] = dev;
  }
  *tab = g_sqrt_dev[at];
  return SP_OK;
}

void release_keys_state() {  // sp_shutdown
  for (int i = 0; i < SP_MAX_CONTEXTS; ++i) {
    if (g_sqrt_dev[i]) {
      DeviceScope on(ctx_at(i).device);
      (void)hipFree(g_sqrt_dev[i]);
      g_sqrt_dev[i] = nullptr;
    }
  }
  g_sqrt_host.reset();
}

// One launch on `st`; takes the library lock for the tables, the profiling bracket and the enqueue.
static int enqueue_keys(bool key, const uint64_t* in, uint64_t* out, uint8_t* status, size_t n, hipStream_t st) {
  ctx_lock lk(ctx().mu);
  const sqrt_tables* tab = nullptr;
  if (out) {
    const int rc = sqrt_tables_for_context(&tab);
    if (rc != SP_OK) return rc;
  }
  const dim3 grid((unsigned)((n + KEYS_TPB - 1) / KEYS_TPB)), block(KEYS_TPB);
  const bool prof = profile_launch_begin(st);
  auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, block, 0, st, in, out, status, n, tab); };
  if (out) key ? launch(stark_keys_kernel<true, true>) : launch(stark_keys_kernel<false, true>);
  else key ? launch(stark_keys_kernel<true, false>) : launch(stark_keys_kernel<false, false>);
  if (prof) profile_launch_end(st, n);
  SP_HIP(hipGetLastError());
  return SP_OK;
}

static int check_args(const char* who, const uint64_t* in, const uint64_t* out, const uint8_t* status, size_t n) {
  if (!in || !status) { set_error(std::string(who) + ": null pointer"); return SP_ERR_BAD_ARGUMENT; }
  if (out && overlap(in, n * 32, out, n * 32)) {
    set_error(std::string(who) + ": input and output overlap");
    return SP_ERR_BAD_ARGUMENT;
  }
  return SP_OK;
}

static int keys_dev(const char* who, bool key, const uint64_t* in, uint64_t* out, uint8_t* status, size_t n, void* stream) {
  CtxByPointer sp_ctx_sel__(in);  // the context of the device these pointers live on
  SP_REQUIRE_READY();
  if (n == 0) return SP_OK;
  const int rc = check_args(who, in, out, status, n);
  if (rc != SP_OK) return rc;
  return enqueue_keys(key, in, out, status, n, (hipStream_t)stream);
}

// Host pointers, on a host lane: one staged round trip (context.hpp StagedTrip).  The caller's `out` goes up with the
// input, so that what the kernel leaves alone - the root of an item that has none - comes back as it was.
static int keys_host(const char* who, bool key, const uint64_t* in, uint64_t* out, uint8_t* status, size_t n) {
  LaneScope ls;
  SP_REQUIRE_READY();
  if (n == 0) return SP_OK;
  int rc = check_args(who, in, out, status, n);
  if (rc != SP_OK) return rc;
  if (ls.open() != SP_OK) return SP_ERR_HIP;
  HostLane& L = *ls.lane;
  const size_t fb = n * 32, ob = out ? fb : 0;
  SP_HIP(L.io.reserve(fb + ob + n + 256));
  char* base = (char*)L.io.ptr;
  uint64_t* din = (uint64_t*)base;
  uint64_t* dout = out ? (uint64_t*)(base + fb) : nullptr;
  uint8_t* dst = (uint8_t*)(base + fb + ob);
  StagedTrip trip(L.hio, fb + 2 * ob + n, L.stream);
  SP_HIP(trip.up(base, {Piece(in, fb), Piece(out, ob)}));
  rc = enqueue_keys(key, din, dout, dst, n, L.stream);
  if (rc != SP_OK) return rc;
  SP_HIP(trip.down(base + fb, {Piece(out, ob), Piece(status, n)}));
  SP_HIP(hipStreamSynchronize(L.stream));
  trip.finish({Piece(out, ob), Piece(status, n)});
  return SP_OK;
}

}  // namespace sp

using namespace sp;

extern "C" {

int sp_felt_sqrt_batch(const uint64_t* a, uint64_t* root, uint8_t* status, size_t n) {
  return keys_host("sp_felt_sqrt_batch", false, a, root, status, n);
}
int sp_felt_sqrt_batch_dev(const uint64_t* a, uint64_t* root, uint8_t* status, size_t n, void* stream) {
  return keys_dev("sp_felt_sqrt_batch_dev", false, a, root, status, n, stream);
}
int sp_stark_key_y_batch(const uint64_t* qx, uint64_t* qy, uint8_t* status, size_t n) {
  return keys_host("sp_stark_key_y_batch", true, qx, qy, status, n);
}
int sp_stark_key_y_batch_dev(const uint64_t* qx, uint64_t* qy, uint8_t* status, size_t n, void* stream) {
  return keys_dev("sp_stark_key_y_batch_dev", true, qx, qy, status, n, stream);
}

}  // extern "C"
