// The P-384 class: ECDSA over secp384r1 under keys given
// with the call -- the reference's ecdsa.Verify(pub, hash, r, s) and
// VerifyAuthenticationTag(m, sig, pubKey) for a key pair made at security
// parameter 384 (sample/authentication/keymanager.go:368-382).  Stateless as
// the inline-key class (§4.13): the calls serialise on the context, take a
// buffer of its rotation and read nothing else of it -- no key, no generator
// table, no use count, no memo.
#include "host_internal.h"
#include "p384_ecc.h"

using namespace mbft_host;

static_assert(mbft::kP384Accept == MBFT_ACCEPT && mbft::kP384Reject == MBFT_REJECT_SIG &&
                  mbft::kP384BadKey == MBFT_BAD_KEY,
              "p384_ecc.h restates the status codes");

namespace {

// SubjectPublicKeyInfo of an uncompressed secp384r1 point, up to the point:
// SEQUENCE(0x76) { SEQUENCE { OID ecPublicKey, OID secp384r1 }, BIT STRING(0x62, 0 unused) { 04 || X || Y } }
const uint8_t kPkixPrefix384[23] = {0x30, 0x76, 0x30, 0x10, 0x06, 0x07, 0x2a, 0x86, 0x48, 0xce, 0x3d, 0x02,
                                    0x01, 0x06, 0x05, 0x2b, 0x81, 0x04, 0x00, 0x22, 0x03, 0x62, 0x00};

// n items on the device -> device status, on stream st: buffer k of the
// rotation as verify_keys_device takes it (free once ev_done[k] has passed,
// marked done again behind the kernel), though the kernel needs no workspace.
int verify_p384_device(mbft_ctx* c, const uint8_t* d_e, const uint8_t* d_r, const uint8_t* d_s, const uint8_t* d_xy,
                       size_t n, uint8_t* d_status, hipStream_t st) {
  if (n == 0) return MBFT_OK;
  const int k = c->pipe;
  c->pipe = (k + 1) % mbft_ctx::kPipe;
  const mbft::P384Plan plan = mbft::verify_p384_plan((long)n, mbft_launch::device_cus());
  HIPCHK(c, hipStreamWaitEvent(st, c->ev_done[k], 0));
  const mbft_launch::P384Batch b{d_e, d_r, d_s, d_xy, (long)n, d_status};
  HIPCHK(c, mbft_launch::verify_p384(b, plan, st));
  HIPCHK(c, hipEventRecord(c->ev_done[k], st));
  return MBFT_OK;
}

// Host buffers in, host status out, on the context's own engine.
int verify_p384_host(mbft_ctx* c, const uint8_t* e, const uint8_t* r, const uint8_t* s, const uint8_t* xy, size_t n,
                     uint8_t* status) {
  if (n == 0) return MBFT_OK;
  HIPCHK(c, c->e.ensure(48 * n));
  HIPCHK(c, c->r.ensure(48 * n));
  HIPCHK(c, c->s.ensure(48 * n));
  HIPCHK(c, c->xy.ensure(96 * n));
  HIPCHK(c, c->status.ensure(n));
  HIPCHK(c, hipMemcpyAsync(c->e.p, e, 48 * n, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->r.p, r, 48 * n, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->s.p, s, 48 * n, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->xy.p, xy, 96 * n, hipMemcpyHostToDevice, c->stream));
  if (const int rc = verify_p384_device(c, c->e.as<uint8_t>(), c->r.as<uint8_t>(), c->s.as<uint8_t>(),
                                        c->xy.as<uint8_t>(), n, c->status.as<uint8_t>(), c->stream))
    return rc;
  HIPCHK(c, hipMemcpyAsync(status, c->status.p, n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return MBFT_OK;
}

}  // namespace

extern "C" {

int mbft_pkix_parse_p384(mbft_ctx* c, const uint8_t* pkix, size_t len, uint8_t xy96[96]) {
  if (!pkix || !xy96) return MBFT_ERR_ARG;
  if (len != 120 || memcmp(pkix, kPkixPrefix384, 23) != 0 || pkix[23] != 0x04)
    return c ? fail(c, MBFT_ERR_KEY, "unsupported PKIX public key (expect uncompressed P-384)") : MBFT_ERR_KEY;
  uint32_t x[12], y[12];
  mbft::p384_words_from_be(x, pkix + 24);
  mbft::p384_words_from_be(y, pkix + 72);
  mbft::fe384 qx, qy;
  if (!mbft::p384_on_curve(qx, qy, x, y))
    return c ? fail(c, MBFT_ERR_KEY, "x509: invalid elliptic curve public key") : MBFT_ERR_KEY;
  memcpy(xy96, pkix + 24, 96);
  return MBFT_OK;
}

int mbft_verify_prehashed_p384_keys(mbft_ctx* c, const uint8_t* e, const uint8_t* r, const uint8_t* s,
                                    const uint8_t* xy, size_t n, uint8_t* status) {
  if (!c || (n && (!e || !r || !s || !xy || !status))) return MBFT_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  if (hipSetDevice(c->device) != hipSuccess) return MBFT_ERR_HIP;
  return verify_p384_host(c, e, r, s, xy, n, status);
}

int mbft_verify_prehashed_p384_keys_device(mbft_ctx* c, const uint8_t* d_e, const uint8_t* d_r, const uint8_t* d_s,
                                           const uint8_t* d_xy, size_t n, uint8_t* d_status, void* hip_stream) {
  if (!c || (n && (!d_e || !d_r || !d_s || !d_xy || !d_status))) return MBFT_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  if (hipSetDevice(c->device) != hipSuccess) return MBFT_ERR_HIP;
  hipStream_t st = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream;
  return verify_p384_device(c, d_e, d_r, d_s, d_xy, n, d_status, st);
}

// PublicAuthenScheme.VerifyAuthenticationTag(m, sig, pk) under P-384 keys, n
// calls: the order of mbft_scheme_verify_flat32 (DER first, then the key --
// which the GPU validates), only the undecided calls travel.
int mbft_scheme_verify_p384_flat32(mbft_ctx* c, const uint8_t* msgs, const uint32_t* msg_off, const uint8_t* tags,
                                   const uint32_t* tag_off, const uint8_t* xy, size_t n, uint8_t* status_out) {
  if (!c || (n && (!msg_off || !tag_off || !xy || !status_out))) return MBFT_ERR_ARG;
  if (n == 0) return MBFT_OK;
  if ((!msgs && msg_off[n] != msg_off[0]) || (!tags && tag_off[n] != tag_off[0])) return MBFT_ERR_ARG;
  std::vector<uint8_t> e, r, s, q, st;
  std::vector<size_t> origin;
  e.reserve(48 * n);
  r.reserve(48 * n);
  s.reserve(48 * n);
  q.reserve(96 * n);
  origin.reserve(n);
  for (size_t i = 0; i < n; i++) {
    if (msg_off[i + 1] < msg_off[i] || tag_off[i + 1] < tag_off[i]) return MBFT_ERR_ARG;
    const size_t msg_len = msg_off[i + 1] - msg_off[i], tag_len = tag_off[i + 1] - tag_off[i];
    uint8_t r48[48], s48[48], e48[48];
    size_t consumed = 0;
    // crypto.go:79-89: DER first (Go panics on error); bytes after the SEQUENCE are ignored
    if (!mbft_der_parse_sig48(tag_len ? tags + tag_off[i] : nullptr, tag_len, r48, s48, &consumed)) {
      status_out[i] = MBFT_MALFORMED_DER;
      continue;
    }
    // md = msg || SHA256("") (crypto.go:121), L = msg_len + 32 bytes; hashToInt for a 384-bit
    // order: the left-most 48 bytes, or -- for messages under 16 bytes -- the whole of md as
    // a big-endian integer, right-aligned (no shift: the order's length is a byte multiple)
    if (msg_len >= 48) {
      memcpy(e48, msgs + msg_off[i], 48);
    } else {
      const size_t take = msg_len + 32 < 48 ? msg_len + 32 : 48;  // bytes of md that count
      memset(e48, 0, 48 - take);
      uint8_t* out = e48 + (48 - take);
      if (msg_len) memcpy(out, msgs + msg_off[i], msg_len);
      memcpy(out + msg_len, kEmptyHash, take - msg_len);
    }
    e.insert(e.end(), e48, e48 + 48);
    r.insert(r.end(), r48, r48 + 48);
    s.insert(s.end(), s48, s48 + 48);
    q.insert(q.end(), xy + 96 * i, xy + 96 * i + 96);
    origin.push_back(i);
  }
  const size_t m = origin.size();
  if (m == 0) return MBFT_OK;
  st.resize(m);
  {
    std::lock_guard<std::mutex> g(c->mu);
    if (hipSetDevice(c->device) != hipSuccess) return MBFT_ERR_HIP;
    if (const int rc = verify_p384_host(c, e.data(), r.data(), s.data(), q.data(), m, st.data())) return rc;
  }
  for (size_t j = 0; j < m; j++) status_out[origin[j]] = st[j];
  return MBFT_OK;
}

}  // extern "C"
