// Batch GenerateMessageAuthenTag for the ECDSA roles (api/api.go:133-144;
// sample/authentication/crypto.go:57-76): the host side of k_sign_tags
// (sign_kernels.hip).  The role's private key lives in a 32-byte device
// buffer from mbft_set_private_key on (zeroed before it is freed: on
// mbft_clear_keys, at destroy, after a failed upload; a replacement is written
// over the zeroed old key); the signer's small generator table is built on first use.
//
// The software USIG (mbft_usig_*): the host side of
// k_usig_uis, replacing the enclave's ecall_usig_create_ui
// (usig/sgx/enclave/usig.c:36-76) and the Go wrapper around it
// (usig/sgx/sgx-usig.go:52-64 CreateUI, :71-79 ID) on hosts without SGX.
// It has NONE of the trusted-hardware guarantee MinBFT's f < n/2 bound rests
// on: whoever controls the host controls the counter.  The instance's key
// lives in a zero-on-free device buffer like the role keys; its counter is
// handed out under the context lock and advanced only after the UIs of a call
// have all come back (usig_run).
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

// ---------------------------------------------------------------------------
// The software USIG.  All of it under c->mu, device set.

// N, big-endian
const uint8_t kOrderN[32] = {0xFF, 0xFF, 0xFF, 0xFF, 0x00, 0x00, 0x00, 0x00, 0xFF, 0xFF, 0xFF,
                             0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xBC, 0xE6, 0xFA, 0xAD, 0xA7, 0x17,
                             0x9E, 0x84, 0xF3, 0xB9, 0xCA, 0xC2, 0xFC, 0x63, 0x25, 0x51};

// 0 < d < N, without an early exit on the key's bytes
bool scalar_in_range(const uint8_t d[32]) {
  uint32_t any = 0;
  int borrow = 0;
  for (int j = 31; j >= 0; j--) {
    any |= d[j];
    borrow = ((int)d[j] - (int)kOrderN[j] - borrow) < 0 ? 1 : 0;
  }
  return any != 0 && borrow == 1;
}

int usig_ready(mbft_ctx* c) {
  if (!c->usig_key) return fail(c, MBFT_ERR_STATE, "no USIG instance (mbft_usig_init)");
  return MBFT_OK;
}

// One CreateUI batch over inputs already on their way to the device: the
// range [next, next + n) is reserved (the context lock is held), the kernel
// runs, the UIs come home, and only when every one of them is there does the
// counter advance.  upload_rc: the outcome of the caller's uploads.  On any
// failure no UI is handed out -- both output buffers are zeroed -- and the
// counter stays, so the same values are signed by a later call and by none
// that left the library.
int usig_run(mbft_ctx* c, int upload_rc, mbft_launch::UsigArgs& a, size_t n, uint8_t* uis,
             uint8_t* ui_len, uint64_t* first_counter) {
  auto device_part = [&]() -> int {
    if (upload_rc) return upload_rc;
    if (n > UINT64_MAX - c->usig_next) return fail(c, MBFT_ERR_STATE, "USIG counter exhausted");
    HIPCHK(c, c->sg_tags.ensure((size_t)MBFT_UI_SLOT * n));
    HIPCHK(c, c->sg_len.ensure(n));
    a.epoch = c->usig_epoch;
    a.first = c->usig_next;
    a.key = static_cast<const uint8_t*>(c->usig_key);
    a.tab = c->sign_tab;
    a.w = c->sign_tab_w;
    a.n = (long)n;
    a.uis = c->sg_tags.as<uint8_t>();
    a.ui_len = c->sg_len.as<uint8_t>();
    HIPCHK(c, mbft_launch::usig_uis(a, c->stream));
    HIPCHK(c, hipMemcpyAsync(uis, a.uis, (size_t)MBFT_UI_SLOT * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(ui_len, a.ui_len, n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < n; i++)
      if (ui_len[i] == 0) return fail(c, MBFT_ERR_STATE, "USIG: an item found no usable nonce");
    return MBFT_OK;
  };
  const int rc = device_part();
  if (rc) {
    (void)hipStreamSynchronize(c->stream);  // no copy may land after the zeroing
    memset(uis, 0, (size_t)MBFT_UI_SLOT * n);
    memset(ui_len, 0, n);
    return rc;
  }
  if (first_counter) *first_counter = c->usig_next;
  c->usig_next += n;  // the UIs are exposed from here on
  return MBFT_OK;
}

void usig_drop(mbft_ctx* c) {
  wipe_free(c, c->usig_key);
  c->usig_next = 0;
  memset(c->usig_ident, 0, sizeof(c->usig_ident));
}

}  // namespace

namespace mbft_host {

int usig_single(mbft_ctx* c, const uint8_t* msg, size_t msg_len, uint8_t* tag_out, size_t tag_cap,
                size_t* tag_len) {
  if (msg_len > 0xFFFFFFFFu) return MBFT_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  if (!c->usig_key) return fail(c, MBFT_ERR_STATE, "no ECDSA private key for role");
  // a UI that does not fit could not be handed out after its counter was
  // spent: the whole slot must fit
  *tag_len = MBFT_UI_SLOT;
  if (tag_cap < MBFT_UI_SLOT) return MBFT_ERR_ARG;
  if (hipSetDevice(c->device) != hipSuccess) return MBFT_ERR_HIP;
  if (int rc = ensure_table(c)) return rc;
  const uint32_t off[2] = {0, (uint32_t)msg_len};
  mbft_launch::UsigArgs a{};
  a.mode = mbft_launch::kUsigFlat;
  auto upload = [&]() -> int {
    HIPCHK(c, c->sg_in.ensure(msg_len ? msg_len : 1));
    HIPCHK(c, c->sg_off.ensure(8));
    if (msg_len) HIPCHK(c, hipMemcpyAsync(c->sg_in.p, msg, msg_len, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->sg_off.p, off, 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // off leaves scope with this call
    return MBFT_OK;
  };
  const int up = upload();
  a.msgs = c->sg_in.as<uint8_t>();
  a.msg_off = c->sg_off.as<uint32_t>();
  uint8_t slot[MBFT_UI_SLOT], len = 0;
  if (int rc = usig_run(c, up, a, 1, slot, &len, nullptr)) return rc;
  memcpy(tag_out, slot, len);
  *tag_len = len;
  return MBFT_OK;
}

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
  usig_drop(c);  // the USIG instance goes with the keys; its epoch stays on record
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

// --- the software USIG -------------------------------------

int mbft_usig_init(mbft_ctx* c, const uint8_t d[32], uint64_t epoch) {
  if (!c || !d) return MBFT_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  if (!scalar_in_range(d)) return fail(c, MBFT_ERR_KEY, "USIG key outside [1, N)");
  if (c->usig_had && epoch == c->usig_last_epoch)
    return fail(c, MBFT_ERR_STATE, "USIG epoch equals the previous instance's");
  if (hipSetDevice(c->device) != hipSuccess) return MBFT_ERR_HIP;
  if (int rc = ensure_table(c)) return rc;
  usig_drop(c);  // an earlier instance ends here, whatever follows
  if (hipMalloc(&c->usig_key, 32) != hipSuccess) {
    (void)hipGetLastError();
    c->usig_key = nullptr;
    return fail(c, MBFT_ERR_NOMEM, "USIG key: out of device memory");
  }
  uint8_t xy[64];
  hipError_t e = hipMemsetAsync(c->usig_key, 0, 32, c->kstream);
  if (e == hipSuccess) e = hipMemcpyAsync(c->usig_key, d, 32, hipMemcpyHostToDevice, c->kstream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->kstream);
  // the public key d G for the identity, by the uniform comb
  if (e == hipSuccess) e = c->sg_tags.ensure(64);
  if (e == hipSuccess)
    e = mbft_launch::sign_pubkey(static_cast<const uint8_t*>(c->usig_key), c->sign_tab, c->sign_tab_w,
                                 c->sg_tags.as<uint8_t>(), c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(xy, c->sg_tags.p, 64, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) {
    usig_drop(c);
    return hip_fail(c, e, "USIG key upload");
  }
  put_be64(c->usig_ident, epoch);
  memcpy(c->usig_ident + 8, kPkixPrefix, 26);
  c->usig_ident[8 + 26] = 0x04;
  memcpy(c->usig_ident + 8 + 27, xy, 64);
  c->usig_epoch = epoch;
  c->usig_next = 1;  // usig.c:40: the first UI carries counter 1
  c->usig_had = true;
  c->usig_last_epoch = epoch;
  return MBFT_OK;
}

int mbft_usig_id(mbft_ctx* c, uint8_t* out, size_t cap, size_t* len) {
  if (!c || !len) return MBFT_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  if (int rc = usig_ready(c)) return rc;
  *len = sizeof(c->usig_ident);
  if (!out || cap < sizeof(c->usig_ident)) return MBFT_ERR_ARG;
  memcpy(out, c->usig_ident, sizeof(c->usig_ident));
  return MBFT_OK;
}

int mbft_usig_next_counter(mbft_ctx* c, uint64_t* counter) {
  if (!c || !counter) return MBFT_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  if (int rc = usig_ready(c)) return rc;
  *counter = c->usig_next;
  return MBFT_OK;
}

int mbft_usig_create_uis_digests(mbft_ctx* c, const uint8_t* digests, size_t n, uint8_t* uis,
                                 uint8_t* ui_len, uint64_t* first_counter) {
  if (!c || !first_counter || (n && (!digests || !uis || !ui_len))) return MBFT_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  if (int rc = usig_ready(c)) return rc;
  if (n == 0) {
    *first_counter = c->usig_next;
    return MBFT_OK;
  }
  if (hipSetDevice(c->device) != hipSuccess) return MBFT_ERR_HIP;
  if (int rc = ensure_table(c)) return rc;
  mbft_launch::UsigArgs a{};
  a.mode = mbft_launch::kUsigDigests;
  auto upload = [&]() -> int {
    HIPCHK(c, c->sg_in.ensure(32 * n));
    HIPCHK(c, hipMemcpyAsync(c->sg_in.p, digests, 32 * n, hipMemcpyHostToDevice, c->stream));
    return MBFT_OK;
  };
  const int up = upload();
  a.digests = c->sg_in.as<uint8_t>();
  return usig_run(c, up, a, n, uis, ui_len, first_counter);
}

int mbft_usig_create_uis_flat(mbft_ctx* c, const uint8_t* msgs, const uint32_t* msg_off, size_t n,
                              uint8_t* uis, uint8_t* ui_len, uint64_t* first_counter) {
  if (!c || !first_counter || (n && (!msg_off || !uis || !ui_len))) return MBFT_ERR_ARG;
  for (size_t i = 0; i < n; i++)
    if (msg_off[i + 1] < msg_off[i]) return MBFT_ERR_ARG;
  const size_t total = n ? msg_off[n] : 0;
  if (total && !msgs) return MBFT_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  if (int rc = usig_ready(c)) return rc;
  if (n == 0) {
    *first_counter = c->usig_next;
    return MBFT_OK;
  }
  if (hipSetDevice(c->device) != hipSuccess) return MBFT_ERR_HIP;
  if (int rc = ensure_table(c)) return rc;
  mbft_launch::UsigArgs a{};
  a.mode = mbft_launch::kUsigFlat;
  auto upload = [&]() -> int {
    HIPCHK(c, c->sg_in.ensure(total ? total : 1));
    HIPCHK(c, c->sg_off.ensure(4 * (n + 1)));
    if (total) HIPCHK(c, hipMemcpyAsync(c->sg_in.p, msgs, total, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->sg_off.p, msg_off, 4 * (n + 1), hipMemcpyHostToDevice, c->stream));
    return MBFT_OK;
  };
  const int up = upload();
  a.msgs = c->sg_in.as<uint8_t>();
  a.msg_off = c->sg_off.as<uint32_t>();
  return usig_run(c, up, a, n, uis, ui_len, first_counter);
}

int mbft_usig_sign_messages_flat(mbft_ctx* c, const mbft_msg_rec* recs, size_t n, const uint8_t* bytes,
                                 size_t nbytes, uint8_t* uis, uint8_t* ui_len, uint64_t* first_counter) {
  if (!c || !first_counter || (n && (!recs || !uis || !ui_len)) || (nbytes && !bytes)) return MBFT_ERR_ARG;
  for (size_t i = 0; i < n; i++) {
    const mbft_msg_rec& m = recs[i];
    // only what carries a UI (core/prepare.go, core/commit.go)
    if (m.type != MBFT_MSG_PREPARE && m.type != MBFT_MSG_COMMIT) return MBFT_ERR_ARG;
    if (m.op_len && (m.op_off > nbytes || m.op_len > nbytes - m.op_off)) return MBFT_ERR_ARG;
  }
  std::lock_guard<std::mutex> g(c->mu);
  if (int rc = usig_ready(c)) return rc;
  if (n == 0) {
    *first_counter = c->usig_next;
    return MBFT_OK;
  }
  if (hipSetDevice(c->device) != hipSuccess) return MBFT_ERR_HIP;
  if (int rc = ensure_table(c)) return rc;
  mbft_launch::UsigArgs a{};
  a.mode = mbft_launch::kUsigRecords;
  auto upload = [&]() -> int {
    HIPCHK(c, c->sg_recs.ensure(sizeof(mbft_msg_rec) * n));
    HIPCHK(c, c->sg_in.ensure(nbytes ? nbytes : 1));
    HIPCHK(c, hipMemcpyAsync(c->sg_recs.p, recs, sizeof(mbft_msg_rec) * n, hipMemcpyHostToDevice, c->stream));
    if (nbytes) HIPCHK(c, hipMemcpyAsync(c->sg_in.p, bytes, nbytes, hipMemcpyHostToDevice, c->stream));
    return MBFT_OK;
  };
  const int up = upload();
  a.recs = c->sg_recs.as<mbft_msg_rec>();
  a.bytes = c->sg_in.as<uint8_t>();
  return usig_run(c, up, a, n, uis, ui_len, first_counter);
}

}  // extern "C"
