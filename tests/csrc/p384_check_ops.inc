// The operations the P-384 test programs expose (tests/csrc/p384_host_check.cpp
// on the host, tests/csrc/p384_check.hip on the device): one table, so both
// run the same calls of p384_fe.h / p384_ecc.h.  Every operand and result is
// an integer of P384_OP_WORDS little-endian 32-bit words.  "raw" operands are
// the value a limb vector holds (below 2^392), taken and returned as they are;
// "plain" ones are residues that the operation takes to Montgomery form and
// back itself.

#define P384_OP_WORDS 14
#define P384_OP_MAX_IN 6
#define P384_OP_MAX_OUT 3

enum P384Op {
  OP_MUL, OP_SQR, OP_ADD, OP_SUB, OP_DBL, OP_TPL, OP_CANON, OP_TOMONT, OP_FROMMONT, OP_INV, OP_EQ, OP_WORDS,
  OP_NMUL, OP_NINV, OP_NREDUCE, OP_U1U2, OP_PADD, OP_PDBL, OP_FINISH, OP_ONCURVE, OP_ITEM, OP_SHAMIR, OP_COUNT
};

struct P384OpInfo {
  const char* name;
  int inputs, outputs;
};
static constexpr P384OpInfo kP384Ops[OP_COUNT] = {
    {"mul", 2, 1},      // raw a, b -> raw fe384_mul
    {"sqr", 1, 1},      // raw a -> raw fe384_sqr
    {"add", 2, 1},      // raw -> raw
    {"sub", 2, 1},      // raw -> raw
    {"dbl", 1, 1},      // raw -> raw
    {"tpl", 1, 1},      // raw -> raw
    {"canon", 1, 1},    // raw -> a mod p
    {"tomont", 1, 1},   // raw -> raw
    {"frommont", 1, 1}, // raw -> raw
    {"inv", 1, 1},      // raw (Montgomery) -> raw (Montgomery)
    {"eq", 2, 1},       // raw a, b -> canon both, 1 where equal
    {"words", 1, 1},    // a < 2^384 -> fe384_from_words, fe384_to_words
    {"nmul", 2, 1},     // raw -> raw fn384_mul
    {"ninv", 1, 1},     // raw (Montgomery mod N) -> raw
    {"nreduce", 1, 1},  // e < 2^384 -> e mod N
    {"u1u2", 3, 2},     // e, r, s -> u1, u2
    {"padd", 6, 3},     // plain X1 Y1 Z1 X2 Y2 Z2 -> plain X3 Y3 Z3
    {"pdbl", 3, 3},     // plain X Y Z -> plain X3 Y3 Z3
    {"finish", 3, 1},   // plain X, Z, r -> 1 where the signature holds
    {"oncurve", 2, 1},  // x, y (any 384-bit words) -> 1 where a point
    {"item", 5, 1},     // e, r, s, x, y -> status
    {"shamir", 4, 3},   // u1, u2, plain qx, qy -> plain X Y Z of u1 G + u2 Q
};

static inline int p384_op_code(const char* name) {
  for (int i = 0; i < OP_COUNT; i++) {
    const char *a = kP384Ops[i].name, *b = name;
    while (*a && *a == *b) a++, b++;
    if (*a == 0 && *b == 0) return i;
  }
  return -1;
}
static inline int p384_op_inputs(int op) { return kP384Ops[op].inputs; }
static inline int p384_op_outputs(int op) { return kP384Ops[op].outputs; }

namespace p384_ops {
using namespace mbft;

// 14 words (value < 2^392) -> limbs as they are, and back (the top limb may
// pass 2^28: a value up to 2^396)
P384_HD void raw_in(fe384& o, const uint32_t w[P384_OP_WORDS]) {
  for (int k = 0; k < NL384; k++) {
    const int bit = LB384 * k, j = bit >> 5, sh = bit & 31;
    const uint64_t two = (uint64_t)w[j] | ((uint64_t)(j + 1 < P384_OP_WORDS ? w[j + 1] : 0u) << 32);
    o.v[k] = (uint32_t)(two >> sh) & LMASK384;
  }
}
P384_HD void raw_out(uint32_t w[P384_OP_WORDS], const fe384& a) {
  uint64_t acc = 0;
  int have = 0, j = 0;
  for (int k = 0; k < NL384; k++) {
    acc |= (uint64_t)a.v[k] << have;
    have += k == NL384 - 1 ? 32 : LB384;
    while (have >= 32 && j < P384_OP_WORDS) {
      w[j++] = (uint32_t)acc;
      acc >>= 32;
      have -= 32;
    }
  }
  while (j < P384_OP_WORDS) {
    w[j++] = (uint32_t)acc;
    acc >>= 32;
  }
}
P384_HD void plain_in(fe384& o, const uint32_t w[P384_OP_WORDS]) {
  raw_in(o, w);
  fe384_to_mont(o, o);
}
P384_HD void plain_out(uint32_t w[P384_OP_WORDS], const fe384& a) {
  fe384 t;
  fe384_from_mont(t, a);
  fe384_canon(t);
  raw_out(w, t);
}
P384_HD void flag_out(uint32_t w[P384_OP_WORDS], uint32_t v) {
  for (int i = 0; i < P384_OP_WORDS; i++) w[i] = 0;
  w[0] = v;
}
}  // namespace p384_ops

// (forced inline: on the device the harness instantiates one kernel per
// operation with `op` a constant, so the switch folds and no kernel calls a
// function)
P384_HD void p384_op_run(int op, const uint32_t (*in)[P384_OP_WORDS], uint32_t (*out)[P384_OP_WORDS]) {
  using namespace mbft;
  using namespace p384_ops;
  fe384 a, b, c;
  switch (op) {
    case OP_MUL: raw_in(a, in[0]); raw_in(b, in[1]); fe384_mul(c, a, b); raw_out(out[0], c); break;
    case OP_SQR: raw_in(a, in[0]); fe384_sqr(c, a); raw_out(out[0], c); break;
    case OP_ADD: raw_in(a, in[0]); raw_in(b, in[1]); fe384_add(c, a, b); raw_out(out[0], c); break;
    case OP_SUB: raw_in(a, in[0]); raw_in(b, in[1]); fe384_sub(c, a, b); raw_out(out[0], c); break;
    case OP_DBL: raw_in(a, in[0]); fe384_dbl(c, a); raw_out(out[0], c); break;
    case OP_TPL: raw_in(a, in[0]); fe384_tpl(c, a); raw_out(out[0], c); break;
    case OP_CANON: raw_in(a, in[0]); fe384_canon(a); raw_out(out[0], a); break;
    case OP_TOMONT: raw_in(a, in[0]); fe384_to_mont(c, a); raw_out(out[0], c); break;
    case OP_FROMMONT: raw_in(a, in[0]); fe384_from_mont(c, a); raw_out(out[0], c); break;
    case OP_INV: raw_in(a, in[0]); fe384_inv(c, a); raw_out(out[0], c); break;
    case OP_EQ:
      raw_in(a, in[0]); raw_in(b, in[1]); fe384_canon(a); fe384_canon(b);
      flag_out(out[0], fe384_eq_canon(a, b) ? 1u : 0u);
      break;
    case OP_WORDS: {
      uint32_t w[12];
      fe384_from_words(a, in[0]);
      fe384_to_words(w, a);
      flag_out(out[0], 0);
      for (int i = 0; i < 12; i++) out[0][i] = w[i];
      break;
    }
    case OP_NMUL: raw_in(a, in[0]); raw_in(b, in[1]); fn384_mul(c, a, b); raw_out(out[0], c); break;
    case OP_NINV: raw_in(a, in[0]); fn384_inv(c, a); raw_out(out[0], c); break;
    case OP_NREDUCE: fe384_from_words(a, in[0]); fn384_reduce(a); raw_out(out[0], a); break;
    case OP_U1U2: {
      uint32_t u1[12], u2[12];
      fn384_u1u2(u1, u2, in[0], in[1], in[2]);
      flag_out(out[0], 0);
      flag_out(out[1], 0);
      for (int i = 0; i < 12; i++) out[0][i] = u1[i], out[1][i] = u2[i];
      break;
    }
    case OP_PADD: {
      pt384 p, q;
      plain_in(p.X, in[0]); plain_in(p.Y, in[1]); plain_in(p.Z, in[2]);
      plain_in(q.X, in[3]); plain_in(q.Y, in[4]); plain_in(q.Z, in[5]);
      p384_add(p, p, q);
      plain_out(out[0], p.X); plain_out(out[1], p.Y); plain_out(out[2], p.Z);
      break;
    }
    case OP_PDBL: {
      pt384 p;
      plain_in(p.X, in[0]); plain_in(p.Y, in[1]); plain_in(p.Z, in[2]);
      p384_dbl(p, p);
      plain_out(out[0], p.X); plain_out(out[1], p.Y); plain_out(out[2], p.Z);
      break;
    }
    case OP_FINISH:
      plain_in(a, in[0]); plain_in(b, in[1]);
      flag_out(out[0], p384_finish(a, b, in[2]) ? 1u : 0u);
      break;
    case OP_ONCURVE: flag_out(out[0], p384_on_curve(a, b, in[0], in[1]) ? 1u : 0u); break;
    case OP_ITEM: flag_out(out[0], p384_verify_item(in[0], in[1], in[2], in[3], in[4])); break;
    case OP_SHAMIR: {
      pt384 acc;
      plain_in(a, in[2]); plain_in(b, in[3]);
      p384_shamir(acc, in[0], in[1], a, b);
      plain_out(out[0], acc.X); plain_out(out[1], acc.Y); plain_out(out[2], acc.Z);
      break;
    }
    default: break;
  }
}
