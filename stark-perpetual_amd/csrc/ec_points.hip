// Batch point arithmetic on the Stark curve: R = k P, R = a EC_GEN + b P, R = P +- Q (ec_mult / ec_add / ec_double of
// math_utils.py:59-100, on the one curve the device knows), one item per lane.
//
// The per-item code is csrc/ec_points.hpp, which the host tests run under g++ as well; k P and b P are ladder.hpp's
// ladder_mul - the code ecdsa_verify_kernel runs - and a EC_GEN is gen_mul.hpp's gathered walk over the context's EC_GEN
// table, the one the verifier walks (the masked table of STARKPERP_SIGN_MASKED=1 is bypassed: include/starkperp.h).
// The two ladder kernels take the launch shape of ecdsa_verify_kernel (256 threads, two waves per SIMD asked of the
// register allocator) and its per-lane table in HBM, keyed by stream.
#include <map>

#include "context.hpp"
#include "ec_points.hpp"
#include "gen_mul.hpp"

namespace sp {

constexpr int EC_TPB = 256;
// Two waves per SIMD asked of the register allocator in the two ladder kernels, as ecdsa_verify_kernel asks
// (SP_VERIFY_WAVES in ecdsa.hip); both stay within 256 VGPRs without scratch.
#define SP_EC_OCCUPANCY __attribute__((amdgpu_waves_per_eu(2, 2)))

// Lanes past the end redo the last item instead of idling (identical reads, identical writes), as ecdsa_verify_kernel
// does; the ladder's table slot is the LANE's, not the item's.
__device__ __forceinline__ void ec_store(uint8_t code, const u256& x, const u256& y, uint64_t* __restrict__ rx,
                                         uint64_t* __restrict__ ry, uint8_t* __restrict__ status, size_t e) {
  status[e] = code;
  if (code != SP_EC_OK) return;
  st_u256(rx + 4 * e, x);
  if (ry) st_u256(ry + 4 * e, y);
}

__global__ void __launch_bounds__(EC_TPB) SP_EC_OCCUPANCY
ec_mult_kernel(const uint64_t* __restrict__ pk, const uint64_t* __restrict__ px, const uint64_t* __restrict__ py,
               uint64_t* __restrict__ rx, uint64_t* __restrict__ ry, uint8_t* __restrict__ status, size_t n,
               int32_t* __restrict__ tab) {
  const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t e = lane < n ? lane : n - 1;
  u256 x, y;
  const uint8_t code = ec_mult_item(ld_u256(pk + 4 * e), ld_u256(px + 4 * e), ld_u256(py + 4 * e), tab,
                                    (size_t)gridDim.x * blockDim.x, lane, x, y);
  ec_store(code, x, y, rx, ry, status, e);
}

__global__ void __launch_bounds__(EC_TPB) SP_EC_OCCUPANCY
ec_lincomb_kernel(const uint64_t* __restrict__ pa, const uint64_t* __restrict__ pb, const uint64_t* __restrict__ px,
                  const uint64_t* __restrict__ py, uint64_t* __restrict__ rx, uint64_t* __restrict__ ry,
                  uint8_t* __restrict__ status, size_t n, const aff_packed* __restrict__ gen, int wbits, int nwin,
                  int32_t* __restrict__ tab) {
  const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t e = lane < n ? lane : n - 1;
  u256 x, y;
  auto gen_mul_of = [&](const u256& a) { return gen_mul_gathered(a, gen, wbits, nwin); };
  const uint8_t code = ec_lincomb_item(ld_u256(pa + 4 * e), ld_u256(pb + 4 * e), ld_u256(px + 4 * e),
                                       ld_u256(py + 4 * e), gen_mul_of, tab, (size_t)gridDim.x * blockDim.x, lane, x, y);
  ec_store(code, x, y, rx, ry, status, e);
}

__global__ void __launch_bounds__(EC_TPB)
ec_add_kernel(const uint64_t* __restrict__ px, const uint64_t* __restrict__ py, const uint64_t* __restrict__ qx,
              const uint64_t* __restrict__ qy, int subtract, uint64_t* __restrict__ rx, uint64_t* __restrict__ ry,
              uint8_t* __restrict__ status, size_t n) {
  size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) e = n - 1;
  u256 x, y;
  const uint8_t code = ec_add_item(ld_u256(px + 4 * e), ld_u256(py + 4 * e), ld_u256(qx + 4 * e), ld_u256(qy + 4 * e),
                                   subtract != 0, x, y);
  ec_store(code, x, y, rx, ry, status, e);
}

// The ladder's per-lane table of the eight odd multiples of P (8 x 36 limbs), per stream; under the library lock.
static std::map<StreamKey, DeviceBuffer> g_ec_tab;

void release_ec_points_state() {  // sp_shutdown
  for (auto& kv : g_ec_tab) kv.second.release();
  g_ec_tab.clear();
}

enum EcOp { EC_MULT, EC_LINCOMB, EC_ADD };
// The arrays of one call: in[] in the order of the entry point's arguments (3, 4, 4 of them).
struct EcArgs {
  EcOp op;
  const uint64_t* in[4];
  int subtract;
  uint64_t *rx, *ry;
  uint8_t* status;
  int inputs() const { return op == EC_MULT ? 3 : 4; }
};

static int check_args(const char* who, const EcArgs& a, size_t n) {
  bool null = !a.rx || !a.status;
  for (int i = 0; i < a.inputs(); ++i) null = null || !a.in[i];
  if (null) { set_error(std::string(who) + ": null pointer"); return SP_ERR_BAD_ARGUMENT; }
  for (int i = 0; i < a.inputs(); ++i) {
    if (overlap(a.in[i], n * 32, a.rx, n * 32) || (a.ry && overlap(a.in[i], n * 32, a.ry, n * 32)) ||
        overlap(a.in[i], n * 32, a.status, n)) {
      set_error(std::string(who) + ": an output overlaps an input");
      return SP_ERR_BAD_ARGUMENT;
    }
  }
  return SP_OK;
}

// One launch on `st`; takes the library lock for the scratch, the profiling bracket and the enqueue.
static int enqueue_ec(const EcArgs& a, size_t n, hipStream_t st) {
  Context& c = ctx();
  ctx_lock lk(c.mu);
  const unsigned blocks = (unsigned)((n + EC_TPB - 1) / EC_TPB);
  int32_t* tab = nullptr;
  if (a.op != EC_ADD) {
    DeviceBuffer& buf = g_ec_tab[stream_key(st)];
    SP_HIP(buf.reserve((size_t)blocks * EC_TPB * 8 * 36 * sizeof(int32_t)));  // one slot per lane
    tab = (int32_t*)buf.ptr;
  }
  const dim3 grid(blocks), block(EC_TPB);
  const bool prof = profile_launch_begin(st);
  if (a.op == EC_MULT)
    hipLaunchKernelGGL(ec_mult_kernel, grid, block, 0, st, a.in[0], a.in[1], a.in[2], a.rx, a.ry, a.status, n, tab);
  else if (a.op == EC_LINCOMB)
    hipLaunchKernelGGL(ec_lincomb_kernel, grid, block, 0, st, a.in[0], a.in[1], a.in[2], a.in[3], a.rx, a.ry, a.status,
                       n, c.gen, c.wbits, c.nwin, tab);
  else
    hipLaunchKernelGGL(ec_add_kernel, grid, block, 0, st, a.in[0], a.in[1], a.in[2], a.in[3], a.subtract, a.rx, a.ry,
                       a.status, n);
  if (prof) profile_launch_end(st, n);
  SP_HIP(hipGetLastError());
  return SP_OK;
}

static int ec_dev(const char* who, const EcArgs& a, size_t n, void* stream) {
  CtxByPointer sp_ctx_sel__(a.in[0]);  // the context of the device these pointers live on
  SP_REQUIRE_READY();
  if (n == 0) return SP_OK;
  const int rc = check_args(who, a, n);
  if (rc != SP_OK) return rc;
  return enqueue_ec(a, n, (hipStream_t)stream);
}

// Host pointers, on a host lane: one staged round trip (context.hpp StagedTrip).  The caller's rx / ry go up with the
// inputs, so that what the kernel leaves alone - the result of an item that is not SP_EC_OK - comes back as it was.
static int ec_host(const char* who, const EcArgs& a, size_t n) {
  LaneScope ls;
  SP_REQUIRE_READY();
  if (n == 0) return SP_OK;
  int rc = check_args(who, a, n);
  if (rc != SP_OK) return rc;
  if (ls.open() != SP_OK) return SP_ERR_HIP;
  HostLane& L = *ls.lane;
  const size_t fb = n * 32, ib = a.inputs() * fb, yb = a.ry ? fb : 0, last = a.inputs() == 4 ? fb : 0;
  SP_HIP(L.io.reserve(ib + fb + yb + n + 256));
  char* base = (char*)L.io.ptr;
  EcArgs d = a;
  for (int i = 0; i < a.inputs(); ++i) d.in[i] = (const uint64_t*)(base + i * fb);
  d.rx = (uint64_t*)(base + ib);
  d.ry = a.ry ? (uint64_t*)(base + ib + fb) : nullptr;
  d.status = (uint8_t*)(base + ib + fb + yb);
  StagedTrip trip(L.hio, ib + 2 * (fb + yb) + n, L.stream);
  SP_HIP(trip.up(base, {Piece(a.in[0], fb), Piece(a.in[1], fb), Piece(a.in[2], fb), Piece(a.in[3], last),
                        Piece(a.rx, fb), Piece(a.ry, yb)}));
  rc = enqueue_ec(d, n, L.stream);
  if (rc != SP_OK) return rc;
  SP_HIP(trip.down(base + ib, {Piece(a.rx, fb), Piece(a.ry, yb), Piece(a.status, n)}));
  SP_HIP(hipStreamSynchronize(L.stream));
  trip.finish({Piece(a.rx, fb), Piece(a.ry, yb), Piece(a.status, n)});
  return SP_OK;
}

}  // namespace sp

using namespace sp;

extern "C" {

int sp_ec_mult_batch(const uint64_t* k, const uint64_t* px, const uint64_t* py, uint64_t* rx, uint64_t* ry,
                     uint8_t* status, size_t n) {
  return ec_host("sp_ec_mult_batch", EcArgs{EC_MULT, {k, px, py, nullptr}, 0, rx, ry, status}, n);
}
int sp_ec_mult_batch_dev(const uint64_t* k, const uint64_t* px, const uint64_t* py, uint64_t* rx, uint64_t* ry,
                         uint8_t* status, size_t n, void* stream) {
  return ec_dev("sp_ec_mult_batch_dev", EcArgs{EC_MULT, {k, px, py, nullptr}, 0, rx, ry, status}, n, stream);
}
int sp_ec_lincomb_batch(const uint64_t* a, const uint64_t* b, const uint64_t* px, const uint64_t* py, uint64_t* rx,
                        uint64_t* ry, uint8_t* status, size_t n) {
  return ec_host("sp_ec_lincomb_batch", EcArgs{EC_LINCOMB, {a, b, px, py}, 0, rx, ry, status}, n);
}
int sp_ec_lincomb_batch_dev(const uint64_t* a, const uint64_t* b, const uint64_t* px, const uint64_t* py,
                            uint64_t* rx, uint64_t* ry, uint8_t* status, size_t n, void* stream) {
  return ec_dev("sp_ec_lincomb_batch_dev", EcArgs{EC_LINCOMB, {a, b, px, py}, 0, rx, ry, status}, n, stream);
}
int sp_ec_add_batch(const uint64_t* px, const uint64_t* py, const uint64_t* qx, const uint64_t* qy, int subtract,
                    uint64_t* rx, uint64_t* ry, uint8_t* status, size_t n) {
  return ec_host("sp_ec_add_batch", EcArgs{EC_ADD, {px, py, qx, qy}, subtract, rx, ry, status}, n);
}
int sp_ec_add_batch_dev(const uint64_t* px, const uint64_t* py, const uint64_t* qx, const uint64_t* qy, int subtract,
                        uint64_t* rx, uint64_t* ry, uint8_t* status, size_t n, void* stream) {
  return ec_dev("sp_ec_add_batch_dev", EcArgs{EC_ADD, {px, py, qx, qy}, subtract, rx, ry, status}, n, stream);
}

}  // extern "C"
