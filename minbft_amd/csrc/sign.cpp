// Batch GenerateMessageAuthenTag for the ECDSA roles (api/api.go:133-144;
// sample/authentication/crypto.go:57-76): the host side of k_sign_tags
// (sign_kernels.hip).  The role's private key lives in a 32-byte device
// buffer from mbft_set_private_key on (zeroed before it is freed: on
// mbft_clear_keys, at destroy, after a failed upload; a replacement is written
// over the zeroed old key); the signer's small generator table is built on first use.
#include "host_internal.h"
#include "sign_kernels.h"

using namespace mbft_host;

namespace {

int role_index(uint32_t role) {
  return role == MBFT_ROLE_REPLICA ? 0 : (role == MBFT_ROLE_CLIENT ? 1 : -1);
}

void wipe_free(mbft_ctx* c, void*& p) {
  if (!p) return;
  (void)hipStreamSynchronize(c->stream);  // a signing kernel in flight reads it
  (void)hipMemsetAsync(p, 0, 32, c->kstream);
  (void)hipStreamSynchronize(c->kstream);
  (void)hipFree(p);
  p = nullptr;
}

// the role's device key, or MBFT_ERR_STATE as the single call reports it
int role_key(mbft_ctx* c, uint32_t role, const uint8_t** key) {
  const int k = role_index(role);
  if (k < 0 || !c->sign_key[k]) return fail(c, MBFT_ERR_STATE, "no ECDSA private key for role");
  *key = static_cast<const uint8_t*>(c->sign_key[k]);
  return MBFT_OK;
}

// the signer's generator table for window c->sign_w (k_table_fill layout)
int ensure_table(mbft_ctx* c) {
  if (c->sign_tab && c->sign_tab_w == c->sign_w) return MBFT_OK;
  const int w = c->sign_w;
  // no signing kernel may read the old table when it is freed: the _device
  // form runs on the caller's stream, so the whole device is drained
  HIPCHK(c, hipDeviceSynchronize());
  if (c->sign_tab) {
    HIPCHK(c, hipFree(c->sign_tab));
    c->sign_tab = nullptr;
  }
  if (hipMalloc(&c->sign_tab, mbft_launch::table_words(w) * 4) != hipSuccess) {
    (void)hipGetLastError();
    c->sign_tab = nullptr;
    return fail(c, MBFT_ERR_NOMEM, "signer table: out of device memory");
  }
  uint32_t *xy = nullptr, *bpts = nullptr;
  HIPCHK(c, hipMalloc(&xy, 64));
  hipError_t e = hipMalloc(&bpts, (size_t)mbft_launch::table_steps(w) * 64);
  if (e == hipSuccess) e = mbft_launch::generator_xy(xy, c->stream);
  if (e == hipSuccess) e = mbft_launch::build_tables(xy, 1, w, bpts, c->sign_tab, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  (void)hipFree(xy);
  if (bpts) (void)hipFree(bpts);
  if (e != hipSuccess) {
    (void)hipFree(c->sign_tab);
    c->sign_tab = nullptr;
    return hip_fail(c, e, "signer table");
  }
  c->sign_tab_w = w;
  return MBFT_OK;
}

// launch over inputs already on the device, tags into the staging, then home
int run_host(mbft_ctx* c, mbft_launch::SignTagArgs& a, size_t n, uint8_t* tags, uint8_t* tag_len) {
  HIPCHK(c, c->sg_tags.ensure((size_t)MBFT_TAG_SLOT * n));
  HIPCHK(c, c->sg_len.ensure(n));
  a.tags = c->sg_tags.as<uint8_t>();
  a.tag_len = c->sg_len.as<uint8_t>();
  a.tab = c->sign_tab;
  a.w = c->sign_tab_w;
  a.n = (long)n;
  HIPCHK(c, mbft_launch::sign_tags(a, c->stream));
  HIPCHK(c, hipMemcpyAsync(tags, a.tags, (size_t)MBFT_TAG_SLOT * n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(tag_len, a.tag_len, n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return MBFT_OK;
}

}  // namespace

namespace mbft_host {

int sign_key_set(mbft_ctx* c, uint32_t role, const uint8_t d[32]) {
  const int k = role_index(role);
  if (k < 0) return MBFT_OK;
  if (!c->sign_key[k]) {
    if (hipMalloc(&c->sign_key[k], 32) != hipSuccess) {
      (void)hipGetLastError();
      c->sign_key[k] = nullptr;
      return fail(c, MBFT_ERR_NOMEM, "private key: out of device memory");
    }
  }
  // a signing kernel in flight on the context's stream reads the old key
  hipError_t e = hipStreamSynchronize(c->stream);
  if (e == hipSuccess) e = hipMemsetAsync(c->sign_key[k], 0, 32, c->kstream);
  if (e == hipSuccess) e = hipMemcpyAsync(c->sign_key[k], d, 32, hipMemcpyHostToDevice, c->kstream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->kstream);
  if (e != hipSuccess) {
    // never leave a half-written key behind: the role has no batch key then
    // (MBFT_ERR_STATE) until a later mbft_set_private_key succeeds
    wipe_free(c, c->sign_key[k]);
    return hip_fail(c, e, "private key upload");
  }
  return MBFT_OK;
}

void sign_keys_wipe(mbft_ctx* c) {
  for (void*& p : c->sign_key) wipe_free(c, p);
}

void sign_destroy(mbft_ctx* c) {
  sign_keys_wipe(c);
  if (c->sign_tab) (void)hipFree(c->sign_tab);
  c->sign_tab = nullptr;
  for (DevBuf* b : {&c->sg_in, &c->sg_off, &c->sg_recs, &c->sg_tags, &c->sg_len}) b->release();
}

}  // namespace mbft_host

extern "C" {

int mbft_set_signer_window(mbft_ctx* c, int wbits) {
  if (!c || wbits < mbft_launch::kSignMinWindow || wbits > mbft_launch::kSignMaxWindow)
    return MBFT_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  c->sign_w = wbits;
  return MBFT_OK;
}

int mbft_generate_tags_prehashed(mbft_ctx* c, uint32_t role, const uint8_t* e, size_t n,
                                 uint8_t* tags, uint8_t* tag_len) {
  if (!c || (n && (!e || !tags || !tag_len))) return MBFT_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  if (hipSetDevice(c->device) != hipSuccess) return MBFT_ERR_HIP;
  mbft_launch::SignTagArgs a{};
  a.mode = mbft_launch::kSignPrehashed;
  if (int rc = role_key(c, role, &a.key0)) return rc;
  if (n == 0) return MBFT_OK;
  if (int rc = ensure_table(c)) return rc;
  HIPCHK(c, c->sg_in.ensure(32 * n));
  HIPCHK(c, hipMemcpyAsync(c->sg_in.p, e, 32 * n, hipMemcpyHostToDevice, c->stream));
  a.e = c->sg_in.as<uint8_t>();
  return run_host(c, a, n, tags, tag_len);
}

int mbft_generate_tags_flat(mbft_ctx* c, uint32_t role, const uint8_t* msgs, const uint32_t* msg_off,
                            size_t n, uint8_t* tags, uint8_t* tag_len) {
  if (!c || (n && (!msg_off || !tags || !tag_len))) return MBFT_ERR_ARG;
  for (size_t i = 0; i < n; i++)
    if (msg_off[i + 1] < msg_off[i]) return MBFT_ERR_ARG;
  const size_t total = n ? msg_off[n] : 0;
  if (total && !msgs) return MBFT_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  if (hipSetDevice(c->device) != hipSuccess) return MBFT_ERR_HIP;
  mbft_launch::SignTagArgs a{};
  a.mode = mbft_launch::kSignFlat;
  if (int rc = role_key(c, role, &a.key0)) return rc;
  if (n == 0) return MBFT_OK;
  if (int rc = ensure_table(c)) return rc;
  HIPCHK(c, c->sg_in.ensure(total ? total : 1));
  HIPCHK(c, c->sg_off.ensure(4 * (n + 1)));
  if (total) HIPCHK(c, hipMemcpyAsync(c->sg_in.p, msgs, total, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->sg_off.p, msg_off, 4 * (n + 1), hipMemcpyHostToDevice, c->stream));
  a.msgs = c->sg_in.as<uint8_t>();
  a.msg_off = c->sg_off.as<uint32_t>();
  return run_host(c, a, n, tags, tag_len);
}

int mbft_generate_tags_prehashed_device(mbft_ctx* c, uint32_t role, const uint8_t* d_e, size_t n,
                                        uint8_t* d_tags, uint8_t* d_tag_len, void* hip_stream) {
  if (!c || (n && (!d_e || !d_tags || !d_tag_len)) || ((uintptr_t)d_e & 3u)) return MBFT_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  if (hipSetDevice(c->device) != hipSuccess) return MBFT_ERR_HIP;
  mbft_launch::SignTagArgs a{};
  a.mode = mbft_launch::kSignPrehashed;
  if (int rc = role_key(c, role, &a.key0)) return rc;
  if (n == 0) return MBFT_OK;
  if (int rc = ensure_table(c)) return rc;
  a.e = d_e;
  a.tags = d_tags;
  a.tag_len = d_tag_len;
  a.tab = c->sign_tab;
  a.w = c->sign_tab_w;
  a.n = (long)n;
  HIPCHK(c, mbft_launch::sign_tags(a, hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream));
  return MBFT_OK;
}

int mbft_sign_messages_flat(mbft_ctx* c, const mbft_msg_rec* recs, size_t n, const uint8_t* bytes,
                            size_t nbytes, uint8_t* tags, uint8_t* tag_len) {
  if (!c || (n && (!recs || !tags || !tag_len)) || (nbytes && !bytes)) return MBFT_ERR_ARG;
  bool need[2] = {false, false};
  for (size_t i = 0; i < n; i++) {
    const mbft_msg_rec& m = recs[i];
    if (m.type == MBFT_MSG_REQUEST) {
      need[1] = true;
    } else if (m.type == MBFT_MSG_REPLY || m.type == MBFT_MSG_REQ_VIEW_CHANGE) {
      need[0] = true;
    } else {
      return MBFT_ERR_ARG;  // PREPARE / COMMIT carry a USIG UI (SGX), or an unknown type
    }
    if (m.type != MBFT_MSG_REQ_VIEW_CHANGE && m.op_len &&
        (m.op_off > nbytes || m.op_len > nbytes - m.op_off))
      return MBFT_ERR_ARG;
  }
  std::lock_guard<std::mutex> g(c->mu);
  if (hipSetDevice(c->device) != hipSuccess) return MBFT_ERR_HIP;
  mbft_launch::SignTagArgs a{};
  a.mode = mbft_launch::kSignRecords;
  if (need[0])
    if (int rc = role_key(c, MBFT_ROLE_REPLICA, &a.key0)) return rc;
  if (need[1])
    if (int rc = role_key(c, MBFT_ROLE_CLIENT, &a.key1)) return rc;
  if (n == 0) return MBFT_OK;
  if (!a.key0) a.key0 = a.key1;  // (no lane reads the role the batch does not hold)
  if (!a.key1) a.key1 = a.key0;
  if (int rc = ensure_table(c)) return rc;
  HIPCHK(c, c->sg_recs.ensure(sizeof(mbft_msg_rec) * n));
  HIPCHK(c, c->sg_in.ensure(nbytes ? nbytes : 1));
  HIPCHK(c, hipMemcpyAsync(c->sg_recs.p, recs, sizeof(mbft_msg_rec) * n, hipMemcpyHostToDevice, c->stream));
  if (nbytes) HIPCHK(c, hipMemcpyAsync(c->sg_in.p, bytes, nbytes, hipMemcpyHostToDevice, c->stream));
  a.recs = c->sg_recs.as<mbft_msg_rec>();
  a.bytes = c->sg_in.as<uint8_t>();
  return run_host(c, a, n, tags, tag_len);
}

}  // extern "C"
