/*
 * ORACLE (test infrastructure, NOT product code): plain-C restatement of the reference's
 * Pedersen hash and Stark-curve ECDSA verification, following the reference ALGORITHM step by
 * step - affine chord/tangent arithmetic with one modular inversion per group operation, LSB-first
 * 252-step hash loop, three 251-step "mimic the AIR" ladders - so it can serve as the CPU baseline
 * and as a fast checker at full workload sizes.  Reference (paths under /root/reference/src):
 *   starkware/crypto/signature/math_utils.py:50-100   div_mod / ec_add / ec_double / ec_mult
 *   starkware/crypto/signature/signature.py:176-260   mimic_ec_mult_air / verify
 *   starkware/crypto/signature/signature.py:296-318   pedersen_hash
 * Parity status: PINNED by tests/test_oracle_c.py against the reference-generated goldens
 * (tests/golden/g1, g2, g4, g6_c2) - the same vectors that pin oracle/ref_py.py.
 * Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may load this library.
 * The section after the batch entry points is the OPTIMISED CPU comparator (windowed fixed-base tables + batched
 * affine additions): same function, a tuned algorithm, pinned by the same goldens - it exists so that
 * the GPU numbers are also compared with a CPU implementation nobody would call naive.
 * After it comes the dense reference of the prover's transforms (NTT / coset LDE / interpolation / coset
 * evaluation / Horner), the restatement of oracle/stark_ref.py at sizes a Python list cannot hold.
 *
 * Build: gcc -O3 -fopenmp -shared -fPIC oracle/starkref.c -o oracle/_build/libstarkref.so
 * Felts are 4 x uint64 little-endian, plain integers.
 */
#include <stdint.h>
#include <string.h>

typedef unsigned __int128 u128;
typedef struct { uint64_t w[4]; } u256;

static const u256 P = {{1ull, 0ull, 0ull, 0x0800000000000011ull}};
static const u256 N = {{0x1e66a241adc64d2full, 0xb781126dcae7b232ull, 0xffffffffffffffffull, 0x0800000000000010ull}};
static const u256 BETA = {{0xf4cdfcb99cee9e89ull, 0x609ad26c15c915c1ull, 0x150e596d72f7a8c5ull, 0x06f21413efbe40deull}};
/* the six independent constant points (pedersen_params.json indices 0, 1, 2, 250, 254, 502) */
static const u256 PTS[6][2] = {
  {{{0x551fde4050ca6804ull, 0x716b0b1022947733ull, 0x00ee1b87eb599f16ull, 0x049ee3eba8c16007ull}},
   {{0xd0405d266e10268aull, 0x4e621062c0e056c1ull, 0xf346d49d06ea0ed3ull, 0x03ca0cfe4b3bc6ddull}}},
  {{{0x3d723d8bc943cfcaull, 0xdeacfd9b0d1819e0ull, 0x7beced415a40f0c7ull, 0x01ef15c18599971bull}},
   {{0x2873000c36e8dc1full, 0xde53ecd11abe43a3ull, 0xb7be4801df46ec62ull, 0x005668060aa49730ull}}},
  {{{0x1080d17957ebe47bull, 0x8fa8120b6d56eb0cull, 0x969c748655fca9e5ull, 0x0234287dcbaffe7full}},
   {{0x6ed0268ee89e5615ull, 0x940135dd7a6c94ccull, 0x1e889527d41f4e39ull, 0x03b056f100f96fb2ull}}},
  {{{0xb7a6932dba8aa378ull, 0x99099ec1de5e3018ull, 0x3f9dab2656558f33ull, 0x04fa56f376c83db3ull}},
   {{0x5168f4e80ff5b54dull, 0x562761f92a7a23b4ull, 0x8113e0c0e47e4401ull, 0x03fa0984c931c9e3ull}}},
  {{{0x3aa372f0bd2d6997ull, 0x40c690c74709e90full, 0x764910f75b45f74bull, 0x04ba4cc166be8decull}},
   {{0x48151f27b24b219cull, 0xcac5c59a5ce5ae7cull, 0x4b971e46c4ede85full, 0x0040301cf5c1751full}}},
  {{{0xd36ff12c49a58202ull, 0x2ca65048d53fb325ull, 0x6e44cca8f61a63bbull, 0x054302dcb0e6cc1cull}},
   {{0x879dcc77e99c2426ull, 0xce98ad783c25561aull, 0xb348046268d8ae25ull, 0x01b77b3e37d13504ull}}},
};

/* ---- 256-bit helpers ---- */
static int is_zero(const u256* a) { return (a->w[0] | a->w[1] | a->w[2] | a->w[3]) == 0; }
static int cmp(const u256* a, const u256* b) {
  for (int i = 3; i >= 0; --i) { if (a->w[i] != b->w[i]) return a->w[i] < b->w[i] ? -1 : 1; }
  return 0;
}
static uint64_t add_to(u256* r, const u256* a, const u256* b) {
  u128 c = 0;
  for (int i = 0; i < 4; ++i) { c += (u128)a->w[i] + b->w[i]; r->w[i] = (uint64_t)c; c >>= 64; }
  return (uint64_t)c;
}
static uint64_t sub_to(u256* r, const u256* a, const u256* b) {
  uint64_t borrow = 0;
  for (int i = 0; i < 4; ++i) {
    u128 d = (u128)a->w[i] - b->w[i] - borrow;
    r->w[i] = (uint64_t)d; borrow = (uint64_t)(d >> 64) & 1;
  }
  return borrow;
}
static void shr1(u256* a, uint64_t top) {
  for (int i = 0; i < 3; ++i) a->w[i] = (a->w[i] >> 1) | (a->w[i + 1] << 63);
  a->w[3] = (a->w[3] >> 1) | (top << 63);
}
static void addmod(u256* r, const u256* a, const u256* b, const u256* m) {
  uint64_t c = add_to(r, a, b);
  if (c || cmp(r, m) >= 0) sub_to(r, r, m);
}
static void submod(u256* r, const u256* a, const u256* b, const u256* m) {
  if (sub_to(r, a, b)) add_to(r, r, m);
}
/* plain a*b mod m: 512-bit schoolbook product, then bitwise-free reduction by repeated shifting
 * would be slow; use Montgomery twice (a*b*R^-1, then * R^2 * R^-1). */
typedef struct { u256 m; uint64_t n0inv; u256 r2; } modulus;
static void mont_mul(u256* out, const u256* a, const u256* b, const modulus* md) {
  uint64_t t[6] = {0, 0, 0, 0, 0, 0};
  for (int i = 0; i < 4; ++i) {
    u128 c = 0;
    for (int j = 0; j < 4; ++j) { c += (u128)a->w[j] * b->w[i] + t[j]; t[j] = (uint64_t)c; c >>= 64; }
    c += t[4]; t[4] = (uint64_t)c; t[5] = (uint64_t)(c >> 64);
    uint64_t q = t[0] * md->n0inv;
    c = (u128)q * md->m.w[0] + t[0]; c >>= 64;
    for (int j = 1; j < 4; ++j) { c += (u128)q * md->m.w[j] + t[j]; t[j - 1] = (uint64_t)c; c >>= 64; }
    c += t[4]; t[3] = (uint64_t)c; t[4] = t[5] + (uint64_t)(c >> 64);
  }
  u256 r = {{t[0], t[1], t[2], t[3]}};
  if (t[4] || cmp(&r, &md->m) >= 0) sub_to(&r, &r, &md->m);
  *out = r;
}
static modulus MP, MN;
static int g_ready = 0;
static void mulmod(u256* r, const u256* a, const u256* b, const modulus* md) {
  u256 t; mont_mul(&t, a, b, md); mont_mul(r, &t, &md->r2, md);
}
/* R^2 mod m by 512 doublings of 1 */
static void init_modulus(modulus* md, const u256* m, uint64_t n0inv) {
  md->m = *m; md->n0inv = n0inv;
  u256 x = {{1, 0, 0, 0}};
  for (int i = 0; i < 512; ++i) addmod(&x, &x, &x, m);
  md->r2 = x;
}
/* modular inverse by the binary extended Euclidean algorithm (the role of sympy's igcdex in
 * math_utils.py:54); returns 0 when a == 0 (gcd != 1 -> the reference asserts). */
static int invmod(u256* r, const u256* a, const u256* m) {
  if (is_zero(a)) return 0;
  u256 u = *a, v = *m, x1 = {{1, 0, 0, 0}}, x2 = {{0, 0, 0, 0}};
  const u256 one = {{1, 0, 0, 0}};
  while (cmp(&u, &one) != 0 && cmp(&v, &one) != 0) {
    while ((u.w[0] & 1) == 0) {
      shr1(&u, 0);
      if (x1.w[0] & 1) { uint64_t c = add_to(&x1, &x1, m); shr1(&x1, c); } else shr1(&x1, 0);
    }
    while ((v.w[0] & 1) == 0) {
      shr1(&v, 0);
      if (x2.w[0] & 1) { uint64_t c = add_to(&x2, &x2, m); shr1(&x2, c); } else shr1(&x2, 0);
    }
    if (cmp(&u, &v) >= 0) { sub_to(&u, &u, &v); submod(&x1, &x1, &x2, m); }
    else { sub_to(&v, &v, &u); submod(&x2, &x2, &x1, m); }
  }
  *r = cmp(&u, &one) == 0 ? x1 : x2;
  return 1;
}

/* ---- affine group law, math_utils.py:59-88; return 0 where the reference asserts ---- */
typedef struct { u256 x, y; } point;
static int ec_add(point* r, const point* a, const point* b) {
  u256 dx, dy, inv, lam, t;
  submod(&dx, &a->x, &b->x, &P);
  if (is_zero(&dx)) return 0;                       /* assert (x1 - x2) % p != 0 */
  submod(&dy, &a->y, &b->y, &P);
  invmod(&inv, &dx, &P);
  mulmod(&lam, &dy, &inv, &MP);
  mulmod(&t, &lam, &lam, &MP);
  submod(&t, &t, &a->x, &P); submod(&t, &t, &b->x, &P);
  u256 y; submod(&y, &a->x, &t, &P); mulmod(&y, &lam, &y, &MP); submod(&y, &y, &a->y, &P);
  r->x = t; r->y = y;
  return 1;
}
static int ec_double(point* r, const point* a) {
  if (is_zero(&a->y)) return 0;                     /* assert y != 0 */
  u256 xx, num, den, inv, lam, t;
  const u256 one = {{1, 0, 0, 0}};
  mulmod(&xx, &a->x, &a->x, &MP);
  addmod(&num, &xx, &xx, &P); addmod(&num, &num, &xx, &P); addmod(&num, &num, &one, &P); /* 3x^2 + alpha */
  addmod(&den, &a->y, &a->y, &P);
  invmod(&inv, &den, &P);
  mulmod(&lam, &num, &inv, &MP);
  mulmod(&t, &lam, &lam, &MP);
  submod(&t, &t, &a->x, &P); submod(&t, &t, &a->x, &P);
  u256 y; submod(&y, &a->x, &t, &P); mulmod(&y, &lam, &y, &MP); submod(&y, &y, &a->y, &P);
  r->x = t; r->y = y;
  return 1;
}

static point CONST_POINTS[506];
static void init_tables(void) {
  if (g_ready) return;
  init_modulus(&MP, &P, 0xffffffffffffffffull);
  init_modulus(&MN, &N, 0xbb6b3c4ce8bde631ull);
  CONST_POINTS[0].x = PTS[0][0]; CONST_POINTS[0].y = PTS[0][1];
  CONST_POINTS[1].x = PTS[1][0]; CONST_POINTS[1].y = PTS[1][1];
  const int start[4] = {2, 250, 254, 502}, count[4] = {248, 4, 248, 4};
  for (int b = 0; b < 4; ++b) {
    point q; q.x = PTS[2 + b][0]; q.y = PTS[2 + b][1];
    for (int j = 0; j < count[b]; ++j) { CONST_POINTS[start[b] + j] = q; point d; ec_double(&d, &q); q = d; }
  }
  g_ready = 1;
}

/* signature.py:300-318.  status: 0 ok, 1 input out of range, 2 "Unhashable input." */
static int pedersen_one(const u256* x, const u256* y, u256* out) {
  if (cmp(x, &P) >= 0 || cmp(y, &P) >= 0) return 1;
  point acc = CONST_POINTS[0];
  const u256* el[2] = {x, y};
  for (int e = 0; e < 2; ++e) {
    u256 s = *el[e];
    for (int j = 0; j < 252; ++j) {
      const point* c = &CONST_POINTS[2 + 252 * e + j];
      if (cmp(&acc.x, &c->x) == 0) return 2;
      if (s.w[0] & 1) { point t; ec_add(&t, &acc, c); acc = t; }
      shr1(&s, 0);
    }
  }
  *out = acc.x;
  return 0;
}

/* signature.py:176-190.  returns 0 on any assertion */
static int mimic_ec_mult_air(point* r, const u256* m_in, const point* pt_in, const point* shift) {
  static const u256 TWO251 = {{0, 0, 0, 0x0800000000000000ull}};
  if (is_zero(m_in) || cmp(m_in, &TWO251) >= 0) return 0;
  u256 m = *m_in; point acc = *shift, pt = *pt_in;
  for (int i = 0; i < 251; ++i) {
    if (cmp(&acc.x, &pt.x) == 0) return 0;
    if (m.w[0] & 1) { point t; if (!ec_add(&t, &acc, &pt)) return 0; acc = t; }
    point d; if (!ec_double(&d, &pt)) return 0; pt = d;
    shr1(&m, 0);
  }
  if (!is_zero(&m)) return 0;
  *r = acc;
  return 1;
}
static int on_curve(const point* q) {
  u256 l, r3, t;
  mulmod(&l, &q->y, &q->y, &MP);
  mulmod(&t, &q->x, &q->x, &MP); mulmod(&r3, &t, &q->x, &MP);
  addmod(&r3, &r3, &q->x, &P); addmod(&r3, &r3, &BETA, &P);
  return cmp(&l, &r3) == 0;
}
/* verify with a point key, signature.py:217-260.  codes as include/starkperp.h SP_VERIFY_* */
static int verify_point(const u256* z, const u256* r, const u256* s, const point* q) {
  static const u256 TWO251 = {{0, 0, 0, 0x0800000000000000ull}};
  if (is_zero(s) || cmp(s, &N) >= 0) return 2;
  u256 w; invmod(&w, s, &N);
  if (is_zero(r) || cmp(r, &TWO251) >= 0) return 3;
  if (is_zero(&w) || cmp(&w, &TWO251) >= 0) return 4;
  if (cmp(z, &TWO251) >= 0) return 5;
  if (!on_curve(q)) return 6;
  point shift = CONST_POINTS[0], mshift = CONST_POINTS[0], zg, rq, b, wb, fin;
  sub_to(&mshift.y, &P, &shift.y);
  if (!mimic_ec_mult_air(&zg, z, &CONST_POINTS[1], &mshift)) return 0;
  if (!mimic_ec_mult_air(&rq, r, q, &shift)) return 0;
  if (!ec_add(&b, &zg, &rq)) return 0;
  if (!mimic_ec_mult_air(&wb, &w, &b, &shift)) return 0;
  if (!ec_add(&fin, &wb, &mshift)) return 0;
  return cmp(r, &fin.x) == 0 ? 1 : 0;
}

/* ---- exported batch entry points ---- */
void cref_pedersen_batch(const uint64_t* x, const uint64_t* y, uint64_t* out, uint8_t* status, size_t n) {
  init_tables();
#pragma omp parallel for schedule(dynamic, 16)
  for (long i = 0; i < (long)n; ++i) {
    u256 a, b, o = {{0, 0, 0, 0}};
    memcpy(&a, x + 4 * i, 32); memcpy(&b, y + 4 * i, 32);
    status[i] = (uint8_t)pedersen_one(&a, &b, &o);
    memcpy(out + 4 * i, &o, 32);
  }
}
/* right fold h = H(e_i, h) from h = e_{n-1} (cairo-lang compute_hash_chain, the consumer behind
 * starkware/cairo/bootloaders/program_hash_test_utils.py:9): serial by nature, one thread.  Returns the OR of the
 * per-link status bytes. */
int cref_pedersen_chain_right(const uint64_t* elems, size_t n, uint64_t* out) {
  init_tables();
  u256 acc;
  int status = 0;
  memcpy(&acc, elems + 4 * (n - 1), 32);
  for (size_t i = n - 1; i-- > 0;) {
    u256 w, o = {{0, 0, 0, 0}};
    memcpy(&w, elems + 4 * i, 32);
    status |= pedersen_one(&w, &acc, &o);
    acc = o;
  }
  memcpy(out, &acc, 32);
  return status;
}
/* full rebuild over 2^height leaves; levels holds 2^(height+1) - 1 felts, leaves first */
void cref_merkle_build(uint64_t* levels, unsigned height) {
  init_tables();
  uint64_t* cur = levels;
  for (size_t n = (size_t)1 << height; n > 1; n >>= 1) {
    uint64_t* nxt = cur + 4 * n;
#pragma omp parallel for schedule(dynamic, 16)
    for (long i = 0; i < (long)(n / 2); ++i) {
      u256 a, b, o = {{0, 0, 0, 0}};
      memcpy(&a, cur + 8 * i, 32); memcpy(&b, cur + 8 * i + 4, 32);
      pedersen_one(&a, &b, &o);
      memcpy(nxt + 4 * i, &o, 32);
    }
    cur = nxt;
  }
}
/* private_key_to_ec_point_on_stark_curve (signature.py:104-106) by the recursion shape of
 * ec_mult (math_utils.py:91-100): double the base while the scalar is even, add on odd. */
void cref_public_key_batch(const uint64_t* d, uint64_t* qx, uint64_t* qy, size_t n) {
  init_tables();
#pragma omp parallel for schedule(dynamic, 4)
  for (long i = 0; i < (long)n; ++i) {
    u256 m; memcpy(&m, d + 4 * i, 32);
    point base = CONST_POINTS[1], pend[512]; int np = 0;
    const u256 one = {{1, 0, 0, 0}};
    while (cmp(&m, &one) != 0) {
      if ((m.w[0] & 1) == 0) { shr1(&m, 0); point t; ec_double(&t, &base); base = t; }
      else { m.w[0] -= 1; pend[np++] = base; }
    }
    point acc = base;
    for (int k = np - 1; k >= 0; --k) { point t; ec_add(&t, &acc, &pend[k]); acc = t; }
    memcpy(qx + 4 * i, &acc.x, 32); memcpy(qy + 4 * i, &acc.y, 32);
  }
}
/* verify with point keys; result codes as SP_VERIFY_* */
void cref_verify_batch(const uint64_t* z, const uint64_t* r, const uint64_t* s, const uint64_t* qx,
                       const uint64_t* qy, uint8_t* result, size_t n) {
  init_tables();
#pragma omp parallel for schedule(dynamic, 1)
  for (long i = 0; i < (long)n; ++i) {
    u256 a, b, c; point q;
    memcpy(&a, z + 4 * i, 32); memcpy(&b, r + 4 * i, 32); memcpy(&c, s + 4 * i, 32);
    memcpy(&q.x, qx + 4 * i, 32); memcpy(&q.y, qy + 4 * i, 32);
    result[i] = (uint8_t)verify_point(&a, &b, &c, &q);
  }
}
/* =============================================================================================
 * Optimised CPU comparator: the SAME function pedersen_hash(x, y), computed
 * the way a tuned CPU library would - NOT the reference's algorithm.  Fixed-base 8-bit windows over the
 * 504-bit string x || y (63 windows x 255 precomputed affine sums of the reference's per-bit points,
 * 1 MiB, built once from CONST_POINTS) and batched affine additions: BATCH hashes advance window by
 * window in lockstep and share ONE modular inversion per window (Montgomery's trick: 3 multiplications
 * per addition for the shared inversion + 3 for the chord rule, instead of the ~250 inversions per
 * hash of the naive path above).  Checked against the same reference goldens (tests/test_oracle_c.py).
 * A window value of 0 skips its addition; an x-collision (acc.x == entry.x, where the reference would
 * raise "Unhashable input." or a windowed sum happens to meet the partial sum) falls back to the
 * naive loop for that hash, whose verdict is the reference's.
 * ============================================================================================= */
#define OPT_WINDOWS 63
#define OPT_BATCH 256
static point* OPT_TABLE = 0; /* [63][256], entry 0 unused; Montgomery form */
static u256 MONT_ONE;
static void to_mont(u256* r, const u256* a) { mont_mul(r, a, &MP.r2, &MP); }
static void from_mont(u256* r, const u256* a) { const u256 one = {{1, 0, 0, 0}}; mont_mul(r, a, &one, &MP); }
extern void* malloc(unsigned long);
static void opt_init(void) {
  init_tables();
  if (OPT_TABLE) return;
#pragma omp critical
  {
    if (!OPT_TABLE) {
      point* tab = (point*)malloc(sizeof(point) * OPT_WINDOWS * 256);
      const u256 one = {{1, 0, 0, 0}};
      to_mont(&MONT_ONE, &one);
      for (int g = 0; g < OPT_WINDOWS; ++g) {
        point* row = tab + 256 * g;
        for (int v = 1; v < 256; ++v) {
          const int low = v & (v - 1);            /* v without its lowest set bit */
          const int bit = __builtin_ctz(v);
          const point* c = &CONST_POINTS[2 + 8 * g + bit];
          if (low == 0) row[v] = *c;
          else ec_add(&row[v], &row[low], c);      /* distinct multiples of independent points: no collision */
        }
      }
      for (int i = 0; i < OPT_WINDOWS * 256; ++i) {
        if ((i & 255) == 0) continue;
        to_mont(&tab[i].x, &tab[i].x); to_mont(&tab[i].y, &tab[i].y);
      }
      OPT_TABLE = tab;
    }
  }
}
/* n <= OPT_BATCH hashes in lockstep; inputs already range-checked by the caller (status 0) */
static void opt_batch(const uint64_t* x, const uint64_t* y, uint64_t* out, uint8_t* status, size_t n) {
  point acc[OPT_BATCH];
  u256 dx[OPT_BATCH], pre[OPT_BATCH];
  const point* ent[OPT_BATCH];
  uint8_t bits[OPT_BATCH][64];
  point shift_m;
  to_mont(&shift_m.x, &CONST_POINTS[0].x); to_mont(&shift_m.y, &CONST_POINTS[0].y);
  for (size_t i = 0; i < n; ++i) {
    acc[i] = shift_m;
    /* the 504-bit string x || y (x: 252 bits), one byte per window */
    uint64_t w[8];
    memcpy(w, x + 4 * i, 32);
    uint64_t yw[4]; memcpy(yw, y + 4 * i, 32);
    /* string = x | (y << 252) */
    uint64_t str[8] = {w[0], w[1], w[2], w[3] | (yw[0] << 60), (yw[0] >> 4) | (yw[1] << 60), (yw[1] >> 4) | (yw[2] << 60),
                       (yw[2] >> 4) | (yw[3] << 60), yw[3] >> 4};
    memcpy(bits[i], str, 64);
  }
  for (int g = 0; g < OPT_WINDOWS; ++g) {
    /* pass 1: denominators and their running product */
    u256 run = MONT_ONE;
    for (size_t i = 0; i < n; ++i) {
      const int v = bits[i][g];
      ent[i] = v ? &OPT_TABLE[256 * g + v] : 0;
      if (status[i] || !ent[i]) { ent[i] = 0; continue; }
      submod(&dx[i], &ent[i]->x, &acc[i].x, &P);
      if (is_zero(&dx[i])) { status[i] = 3; ent[i] = 0; continue; }  /* collision: redo this hash naively */
      pre[i] = run;
      mont_mul(&run, &run, &dx[i], &MP);
    }
    /* one inversion for the whole batch (plain inverse of the Montgomery value, then back to Montgomery) */
    u256 plain, inv;
    from_mont(&plain, &run);
    if (!invmod(&inv, &plain, &P)) continue;  /* nothing to add in this window */
    to_mont(&inv, &inv);
    /* pass 2: individual inverses, chord rule */
    for (size_t k = n; k-- > 0;) {
      if (!ent[k]) continue;
      u256 idx, lam, t, yy;
      mont_mul(&idx, &inv, &pre[k], &MP);
      mont_mul(&inv, &inv, &dx[k], &MP);
      submod(&t, &ent[k]->y, &acc[k].y, &P);
      mont_mul(&lam, &t, &idx, &MP);
      mont_mul(&t, &lam, &lam, &MP);
      submod(&t, &t, &acc[k].x, &P); submod(&t, &t, &ent[k]->x, &P);
      submod(&yy, &acc[k].x, &t, &P); mont_mul(&yy, &lam, &yy, &MP); submod(&yy, &yy, &acc[k].y, &P);
      acc[k].x = t; acc[k].y = yy;
    }
  }
  for (size_t i = 0; i < n; ++i) {
    u256 o = {{0, 0, 0, 0}};
    if (status[i] == 0) from_mont(&o, &acc[i].x);
    else if (status[i] == 3) {
      u256 a, b; memcpy(&a, x + 4 * i, 32); memcpy(&b, y + 4 * i, 32);
      status[i] = (uint8_t)pedersen_one(&a, &b, &o);
    }
    memcpy(out + 4 * i, &o, 32);
  }
}
void cref_opt_pedersen_batch(const uint64_t* x, const uint64_t* y, uint64_t* out, uint8_t* status, size_t n) {
  opt_init();
  const long nb = (long)((n + OPT_BATCH - 1) / OPT_BATCH);
#pragma omp parallel for schedule(dynamic, 1)
  for (long b = 0; b < nb; ++b) {
    const size_t lo = (size_t)b * OPT_BATCH, cnt = n - lo < OPT_BATCH ? n - lo : OPT_BATCH;
    for (size_t i = 0; i < cnt; ++i) {
      u256 a, c; memcpy(&a, x + 4 * (lo + i), 32); memcpy(&c, y + 4 * (lo + i), 32);
      status[lo + i] = (cmp(&a, &P) >= 0 || cmp(&c, &P) >= 0) ? 1 : 0;
    }
    opt_batch(x + 4 * lo, y + 4 * lo, out + 4 * lo, status + lo, cnt);
  }
}
extern void free(void*);
/* full rebuild with the optimised hash; levels: 2^(height+1) - 1 felts, leaves first */
void cref_opt_merkle_build(uint64_t* levels, unsigned height) {
  opt_init();
  uint64_t* cur = levels;
  for (size_t n = (size_t)1 << height; n > 1; n >>= 1) {
    uint64_t* nxt = cur + 4 * n;
    const size_t m = n / 2;
    uint64_t* xs = (uint64_t*)malloc(64 * m + 64);
    uint64_t* ys = xs + 4 * m;
    uint8_t* st = (uint8_t*)malloc(m + 1);
    for (size_t i = 0; i < m; ++i) { memcpy(xs + 4 * i, cur + 8 * i, 32); memcpy(ys + 4 * i, cur + 8 * i + 4, 32); }
    cref_opt_pedersen_batch(xs, ys, nxt, st, m);
    free(xs); free(st);
    cur = nxt;
  }
}

int cref_max_threads(void) {
#ifdef _OPENMP
  extern int omp_get_max_threads(void);
  return omp_get_max_threads();
#else
  return 1;
#endif
}

/* =============================================================================================
 * Dense reference of the prover-side transforms over GF(p) (oracle/stark_ref.py ntt / intt / lde at sizes a
 * Python list cannot hold): plain radix-2 Cooley-Tukey, a bit-reversal permutation followed by log_n
 * decimation-in-time stages, every value canonical after every butterfly (mulmod / addmod / submod above),
 * OpenMP over the butterflies of a stage.  Checked against stark_ref.py at small sizes and against Horner
 * evaluation (tf_horner below: the definition) at large ones, tests/test_transform_ref_cpu.py.
 * ============================================================================================= */
static void tf_init(void) {
  if (g_ready) return;
#pragma omp critical(tf_init_tables)
  init_tables();
}
/* base^e for a 256-bit exponent, square and multiply from the top bit */
static void tf_pow(u256* r, const u256* base, const u256* e) {
  u256 acc = {{1, 0, 0, 0}};
  for (int i = 255; i >= 0; --i) {
    mulmod(&acc, &acc, &acc, &MP);
    if ((e->w[i >> 6] >> (i & 63)) & 1) mulmod(&acc, &acc, base, &MP);
  }
  *r = acc;
}
static void tf_pow_small(u256* r, const u256* base, uint64_t e) {
  const u256 ee = {{e, 0, 0, 0}};
  tf_pow(r, base, &ee);
}
/* 3^((p - 1) >> log_n): the primitive 2^log_n-th root of unity of stark_ref.root_of_unity */
static void tf_root(u256* r, unsigned log_n) {
  u256 e = P;
  e.w[0] -= 1;
  for (unsigned i = 0; i < log_n; ++i) shr1(&e, 0);
  const u256 three = {{3, 0, 0, 0}};
  tf_pow(r, &three, &e);
}
/* out[k] = base^k, k < count: blocks of 1024 consecutive powers, each started by its own exponentiation */
static void tf_powers(u256* out, size_t count, const u256* base) {
  const long nblk = (long)((count + 1023) / 1024);
#pragma omp parallel for schedule(static)
  for (long b = 0; b < nblk; ++b) {
    const size_t lo = (size_t)b * 1024, hi = lo + 1024 < count ? lo + 1024 : count;
    u256 cur;
    tf_pow_small(&cur, base, (uint64_t)lo);
    for (size_t k = lo; k < hi; ++k) { out[k] = cur; mulmod(&cur, &cur, base, &MP); }
  }
}
static size_t tf_bitrev(size_t i, unsigned log_n) {
  size_t r = 0;
  for (unsigned b = 0; b < log_n; ++b) r |= ((i >> b) & 1) << (log_n - 1 - b);
  return r;
}
static void tf_permute(u256* a, unsigned log_n) {
  const long n = (long)1 << log_n;
#pragma omp parallel for schedule(static)
  for (long i = 0; i < n; ++i) {
    const size_t r = tf_bitrev((size_t)i, log_n);
    if ((size_t)i < r) { const u256 t = a[i]; a[i] = a[r]; a[r] = t; }
  }
}
/* a[i] <- sum_k a[k] w^(i k), natural order on both sides; w a primitive 2^log_n-th root of unity.  0 on success. */
static int tf_transform(u256* a, unsigned log_n, const u256* w) {
  if (log_n == 0) return 0;
  const size_t n = (size_t)1 << log_n, half = n >> 1;
  u256* tw = (u256*)malloc(sizeof(u256) * half);
  if (!tw) return 1;
  tf_powers(tw, half, w);
  tf_permute(a, log_n);
  for (unsigned s = 1; s <= log_n; ++s) {
    const size_t h = (size_t)1 << (s - 1);
#pragma omp parallel for schedule(static)
    for (long b = 0; b < (long)half; ++b) {
      const size_t j = (size_t)b & (h - 1), i0 = (((size_t)b >> (s - 1)) << s) | j, i1 = i0 + h;
      u256 t, lo = a[i0];
      mulmod(&t, &a[i1], &tw[j << (log_n - s)], &MP);
      addmod(&a[i0], &lo, &t, &P);
      submod(&a[i1], &lo, &t, &P);
    }
  }
  free(tw);
  return 0;
}
static void tf_scale_all(u256* a, size_t n, const u256* f) {
#pragma omp parallel for schedule(static)
  for (long i = 0; i < (long)n; ++i) mulmod(&a[i], &a[i], f, &MP);
}
/* 1 / 2^log_n */
static void tf_inv_n(u256* r, unsigned log_n) {
  const u256 two = {{2, 0, 0, 0}};
  u256 n;
  tf_pow_small(&n, &two, log_n);
  invmod(r, &n, &P);
}

/* In place.  inverse == 0: evaluations of sum a[k] x^k at w^i (stark_ref.ntt); otherwise the coefficients of the
 * interpolant of a[] over <w>, 1/n included (stark_ref.intt).  0 on success, 1 out of memory. */
int cref_ntt(uint64_t* data, unsigned log_n, int inverse) {
  tf_init();
  u256* a = (u256*)data;
  u256 w;
  tf_root(&w, log_n);
  if (inverse) { u256 wi; invmod(&wi, &w, &P); w = wi; }
  if (tf_transform(a, log_n, &w)) return 1;
  if (inverse) { u256 f; tf_inv_n(&f, log_n); tf_scale_all(a, (size_t)1 << log_n, &f); }
  return 0;
}
/* scratch[k] = coef[k] * shift^k for k < n, 0 for n <= k < m */
static int tf_shift_pad(u256* out, const u256* coef, size_t n, size_t m, const u256* shift) {
  u256* pw = (u256*)malloc(sizeof(u256) * n);
  if (!pw) return 1;
  tf_powers(pw, n, shift);
#pragma omp parallel for schedule(static)
  for (long k = 0; k < (long)n; ++k) mulmod(&out[k], &coef[k], &pw[k], &MP);
  free(pw);
  if (m > n) memset(out + n, 0, sizeof(u256) * (m - n));
  return 0;
}
/* One column of stark_ref.lde: the interpolant of in[] over <w_n>, evaluated on shift * <w_m>, m = n << log_blowup. */
int cref_lde(const uint64_t* in, uint64_t* out, unsigned log_n, unsigned log_blowup, const uint64_t* shift) {
  tf_init();
  const size_t n = (size_t)1 << log_n, m = n << log_blowup;
  u256* coef = (u256*)malloc(sizeof(u256) * n);
  if (!coef) return 1;
  memcpy(coef, in, sizeof(u256) * n);
  u256 sh;
  memcpy(&sh, shift, 32);
  int rc = cref_ntt((uint64_t*)coef, log_n, 1);
  if (!rc) rc = tf_shift_pad((u256*)out, coef, n, m, &sh);
  free(coef);
  if (!rc) rc = cref_ntt(out, log_n + log_blowup, 0);
  return rc;
}
/* include/starkperp.h sp_interpolate_dev: out[bitrev(k)] = n c_k = sum_i in[i] w^(-i k) - the coefficient WITHOUT its
 * 1/n (sp_coset_eval_dev's table carries it), stored at the bit-reversed index. */
int cref_interpolate(const uint64_t* in, uint64_t* out, unsigned log_n) {
  tf_init();
  const size_t n = (size_t)1 << log_n;
  u256 w, wi;
  tf_root(&w, log_n);
  invmod(&wi, &w, &P);
  memcpy(out, in, sizeof(u256) * n);
  if (tf_transform((u256*)out, log_n, &wi)) return 1;
  tf_permute((u256*)out, log_n);
  return 0;
}
/* include/starkperp.h sp_coset_eval_dev: coef as cref_interpolate leaves it -> the interpolant on shift * <w_n>. */
int cref_coset_eval(const uint64_t* coef, uint64_t* out, unsigned log_n, const uint64_t* shift) {
  tf_init();
  const size_t n = (size_t)1 << log_n;
  u256* c = (u256*)malloc(sizeof(u256) * n);
  if (!c) return 1;
  memcpy(c, coef, sizeof(u256) * n);
  tf_permute(c, log_n);
  u256 f, sh;
  tf_inv_n(&f, log_n);
  tf_scale_all(c, n, &f);
  memcpy(&sh, shift, 32);
  int rc = tf_shift_pad((u256*)out, c, n, n, &sh);
  free(c);
  if (!rc) rc = cref_ntt(out, log_n, 0);
  return rc;
}
/* out[q] = sum_k coef[k] x_q^k by Horner's rule: the definition the transforms are checked against */
void cref_horner(const uint64_t* coef, size_t n, const uint64_t* points, size_t k, uint64_t* out) {
  tf_init();
  const u256* c = (const u256*)coef;
#pragma omp parallel for schedule(dynamic, 1)
  for (long q = 0; q < (long)k; ++q) {
    u256 x, acc = {{0, 0, 0, 0}};
    memcpy(&x, points + 4 * q, 32);
    for (size_t i = n; i-- > 0;) { mulmod(&acc, &acc, &x, &MP); addmod(&acc, &acc, &c[i], &P); }
    memcpy(out + 4 * q, &acc, 32);
  }
}
