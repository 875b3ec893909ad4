// The composition value of a prove_builtins proof at opened points (sp_builtins_eval_points_dev): the sum over the
// present segments - Pedersen, ECDSA, rc16 - of each segment's composition at one LDE position, from the two opened
// phase-1 rows and, for rc16, the two opened values of the second-phase column.  Everything a lane of the kernel of
// verify_builtins.hip does, and the argument rules of the call.  Like verify.hpp this needs no HIP: a plain C++
// compiler builds it for tests/host/builtins_verify_shim.cpp, which replays the launch plan over host arrays.
//
// The Pedersen and ECDSA parts are points_body_pedersen and points_body_ecdsa of verify.hpp as they are.  The rc16
// part is new here: it is the first point body that needs the coset point x itself.  The dense call reads three
// tables of M felts (x - g^(n-1), its inverse, 1 / (x - 1)); a lane derives x = shift w_M^pos by square-and-multiply,
// as fri_check_item does, and takes both inverses from ONE fe_inv of the product of the two denominators.  Memory
// follows the proof, not the trace: nothing proportional to M is built or read.
#pragma once
#include "verify.hpp"

namespace sp {

// ---- the segments (values of SP_SEG_* in include/starkperp.h), in the column order of a combined trace ----
constexpr unsigned BSEG_PEDERSEN = 1, BSEG_ECDSA = 2, BSEG_RC16 = 4, BSEG_ALL = 7;
constexpr unsigned BSEG_MAX = 3;
constexpr unsigned RC16_N_COLS = 3, RC16_N_ALPHA = 8, RC16_MIN_LOG_N = 3, RC16_MAX_LOG_N = 24, RC16_PER_LEN = 32;

struct BuiltinsShape {
  unsigned n_segs;   // present segments = waves of a block
  unsigned n_cols;   // felts of one opened phase-1 row
  unsigned n_alpha, min_log_n, max_log_n;
};
struct BuiltinsWave {
  unsigned seg, col0, alpha0;  // BSEG_* of the wave's segment (0: none), its first column in the row, its first alpha
};
// Plain scalar code on purpose (no array indexed by the wave): the kernel evaluates it per wave.
SP_HD BuiltinsWave builtins_wave(unsigned segments, unsigned wave, BuiltinsShape* shape = nullptr) {
  BuiltinsWave w = {0, 0, 0};
  BuiltinsShape s = {0, 0, 0, 0, VERIFY_MAX_LOG_N};
  auto put = [&](unsigned bit, unsigned cols, unsigned alphas, unsigned lo) {
    if (!(segments & bit)) return;
    if (s.n_segs == wave) w = BuiltinsWave{bit, s.n_cols, s.n_alpha};
    ++s.n_segs;
    s.n_cols += cols;
    s.n_alpha += alphas;
    if (lo > s.min_log_n) s.min_log_n = lo;
  };
  put(BSEG_PEDERSEN, 4, 11, 9);  // verify_air_shape(VAIR_PEDERSEN)
  put(BSEG_ECDSA, 10, 26, 10);   // verify_air_shape(VAIR_ECDSA)
  put(BSEG_RC16, RC16_N_COLS, RC16_N_ALPHA, RC16_MIN_LOG_N);
  if (segments & BSEG_RC16) s.max_log_n = RC16_MAX_LOG_N;  // the dense rc16 call's bound
  if (shape) *shape = s;
  return w;
}
SP_HD BuiltinsShape builtins_shape(unsigned segments) {
  BuiltinsShape s;
  builtins_wave(segments, 0, &s);
  return s;
}

// ---- argument rules: nullptr, or the text for sp_last_error.  The first takes no pointer; the second runs with
// n_points > 0 and reads z_host only when rc16 is present ----
SP_HD const char* builtins_check_args(unsigned segments, unsigned log_n, uint64_t rc_min, uint64_t rc_max,
                                      size_t n_points) {
  if (segments < 1 || segments > BSEG_ALL) return "segments outside 1 .. 7 (SP_SEG_PEDERSEN | SP_SEG_ECDSA | SP_SEG_RC16)";
  const BuiltinsShape sh = builtins_shape(segments);
  if (log_n < sh.min_log_n || log_n > sh.max_log_n) return "log_n out of range for these segments";
  if ((segments & BSEG_RC16) && (rc_min > rc_max || rc_max > 0xffff)) return "bad limb range (rc_min <= rc_max <= 0xffff)";
  if (n_points > VERIFY_MAX_ITEMS) return "more than 2^30 points";
  return nullptr;
}
SP_HD const char* builtins_check_pointers(unsigned segments, const uint64_t* per_pedersen, const uint64_t* per_ecdsa,
                                          const uint64_t* per_rc16, const uint64_t* alphas_host,
                                          const uint64_t* shift_host, const uint64_t* z_host, const uint64_t* pos,
                                          const uint64_t* cur, const uint64_t* nxt, const uint64_t* pcur,
                                          const uint64_t* pnxt, const uint64_t* out, const uint8_t* status) {
  bool null = !alphas_host || !shift_host || !pos || !cur || !nxt || !out || !status;
  if (segments & BSEG_PEDERSEN) null = null || !per_pedersen;
  if (segments & BSEG_ECDSA) null = null || !per_ecdsa;
  if (segments & BSEG_RC16) null = null || !per_rc16 || !z_host || !pcur || !pnxt;
  if (null) return "a NULL pointer with points to evaluate";
  if ((segments & BSEG_RC16) && !vf_is_felt(z_host)) return "bad z (not below p)";
  if (!vf_is_felt(shift_host)) return "bad shift (not below p)";
  return nullptr;
}

// ---- the rc16 composition at one point ----
struct Rc16PointParams {
  fe alpha[8];                  // Montgomery
  fe zinv[4];                   // air_zinv(times_r2 = false): Montgomery form of 1 / (x^n - 1) for pos mod 4
  fe z, rc_min, rc_max, two16;  // Montgomery
  fe shift, w, g_last;          // Montgomery: the coset shift, the primitive M-th root of unity, g^(n-1) = 1 / g
};
// zinv is left to the caller (air_zinv of stark.hip in the library)
SP_HD void rc16_point_params(unsigned log_n, const uint64_t* alphas_host, const uint64_t* shift_host,
                             const uint64_t* z_host, uint64_t rc_min, uint64_t rc_max, Rc16PointParams* prm) {
  for (unsigned k = 0; k < RC16_N_ALPHA; ++k) prm->alpha[k] = fe_to_mont(vf_fe(alphas_host + 4 * k));
  prm->z = fe_to_mont(vf_fe(z_host));
  prm->rc_min = fe_to_mont(fe{{(int32_t)rc_min, 0, 0, 0, 0, 0, 0, 0, 0}});
  prm->rc_max = fe_to_mont(fe{{(int32_t)rc_max, 0, 0, 0, 0, 0, 0, 0, 0}});
  prm->two16 = fe_to_mont(fe{{1 << 16, 0, 0, 0, 0, 0, 0, 0, 0}});
  prm->shift = fe_to_mont(vf_fe(shift_host));
  prm->w = verify_root_of_unity(log_n + 2);
  prm->g_last = fe_inv(verify_root_of_unity(log_n));
}

// air_body_rc16 (air_bodies.hpp) at one opened point - the function air_eval_rc16_kernel (builtins.hip) evaluates,
// C0 .. C7 of oracle/stark_ref.rc16_constraint_values combined as rc16_composition_value.  Like the dense kernel, and
// unlike the four bodies of verify.hpp, it keeps its Montgomery factors itself: every operand is loaded to Montgomery
// form (the kernel's ld_plain_m), zinv carries no R^2, and the result leaves through fe_from_mont.  Where the kernel
// reads d_last = x - g^(n-1), inv_last = 1 / d_last and inv_first = 1 / (x - 1) from tables over the coset, this
// derives x = shift w^pos (log_m squarings, most significant bit first) and one inversion of d_last (x - 1).  Neither
// denominator vanishes: 1 and g^(n-1) lie on the trace domain, and a shift with shift^(4n) = 1 is refused.
struct Rc16PointRow {
  const uint64_t *row, *p;  // the opened phase-1 row (a, acc, s) and, as column 3, the opened second-phase value
  SP_HD fe operator()(int c) const { return fe_to_mont(vf_fe(c < 3 ? row + 4 * c : p)); }
};
struct Rc16PointPeriodic {
  const uint64_t* per;
  uint64_t at;  // pos mod 32
  SP_HD fe operator()(int c) const { return fe_to_mont(vf_fe(per + 4 * (32 * c + at))); }
};
SP_HD fe points_body_rc16(const uint64_t* cur, const uint64_t* nxt, const uint64_t* pcur, const uint64_t* pnxt,
                          const uint64_t* per, uint64_t pos, unsigned log_m, const Rc16PointParams& prm) {
  fe pw = FE_ONE_M;  // w^pos
  for (int bit = (int)log_m - 1; bit >= 0; --bit) {
    pw = fe_sqr(pw);
    if ((pos >> bit) & 1) pw = fe_mul(pw, prm.w);
  }
  const fe x = fe_mul(prm.shift, pw);
  const fe dl = fe_carry(fe_sub(x, prm.g_last));
  const fe d1 = fe_carry(fe_sub(x, FE_ONE_M));
  const fe inv = fe_inv(fe_mul(dl, d1));
  const fe il = fe_mul(inv, d1), i1 = fe_mul(inv, dl);
  return fe_from_mont(air_body_rc16(Rc16PointRow{cur, pcur}, Rc16PointRow{nxt, pnxt}, Rc16PointPeriodic{per, pos & 31},
                                    prm.alpha, prm.zinv[pos & 3], prm.z, prm.rc_min, prm.rc_max, prm.two16, dl, il, i1));
}

// ---- one point, one segment: what ONE wave of a block does for its lane's point ----
struct BuiltinsPointsArgs {
  unsigned segments, log_n;
  const uint64_t *per_pedersen, *per_ecdsa, *per_rc16;
  size_t n_points;
  const uint64_t *pos, *cur, *nxt, *pcur, *pnxt;
  uint64_t* out;
  uint8_t* status;
};
// The wave of segment w.seg (builtins_wave) evaluates it at point i: the canonical value of that segment's
// composition, or zero with *ok = false when pos[i] >= M or a felt this segment reads - its columns of the two rows
// and, for rc16, pcur[i] and pnxt[i] - is not below p.  The periodic tables are read at pos mod their length only.
SP_HD fe builtins_segment_value(const BuiltinsPointsArgs& g, const BuiltinsWave& w, unsigned n_cols,
                                const PointsAirParams& ped, const PointsAirParams& ecd, const Rc16PointParams& rc,
                                size_t i, bool* ok_out) {
  const unsigned seg = w.seg;
  const unsigned cols = seg == BSEG_PEDERSEN ? 4u : seg == BSEG_ECDSA ? 10u : RC16_N_COLS;
  const uint64_t p = g.pos[i];
  const uint64_t* c = g.cur + 4 * (i * n_cols + w.col0);
  const uint64_t* n = g.nxt + 4 * (i * n_cols + w.col0);
  bool ok = p < ((uint64_t)4 << g.log_n);
  for (unsigned k = 0; k < cols; ++k) ok = ok & vf_is_felt(c + 4 * k) & vf_is_felt(n + 4 * k);
  if (seg == BSEG_RC16) ok = ok & vf_is_felt(g.pcur + 4 * i) & vf_is_felt(g.pnxt + 4 * i);
  *ok_out = ok;
  if (!ok) return FE_ZERO;
  if (seg == BSEG_PEDERSEN) return points_body_pedersen(c, n, g.per_pedersen, p, ped);
  if (seg == BSEG_ECDSA) return points_body_ecdsa(c, n, g.per_ecdsa, p, ecd);
  return points_body_rc16(c, n, g.pcur + 4 * i, g.pnxt + 4 * i, g.per_rc16, p, g.log_n + 2, rc);
}
// Wave 0 after the barrier, with `sum` the limb-wise fe_add of the present segments' canonical parts (at most three,
// below 3 p) and `ok` the AND of their flags: the sum mod p - what sp_felt_add_dev makes of the dense columns - or
// zero and OUT_OF_RANGE when any wave flagged the point.
SP_HD void builtins_store(const fe& sum, bool ok, size_t i, uint64_t* out, uint8_t* status) {
  u256 r;
  for (int k = 0; k < 8; ++k) r.w[k] = 0;
  if (ok) r = fe_pack(fe_canon(sum));
  vf_store(out + 4 * i, r);
  status[i] = ok ? VERIFY_OK : VERIFY_OUT_OF_RANGE;
}

}  // namespace sp
