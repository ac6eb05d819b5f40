// Test-only harness (tests/test_gpu_tables.py, tests/test_gpu_ninv.py): calls
// the library's own host-side launchers (minbft_amd/csrc/kernels.h, linked
// from libminbft_amd.so) on caller-given host arrays and hands their raw
// device results back, so that Python can check every comb-table entry and
// every s^-1 plane against big-integer arithmetic -- and runs the verifier's
// large path (mbft_launch::verify, verify_keys) on a grid of the caller's
// choosing, handing back statuses, both queues and the guard lines
// (tests/test_gpu_verify_passes.py).  Built into
// tests/liblaunch_check.so by __graft_entry__.build(); never part of the
// product library.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../minbft_amd/csrc/kernels.h"

namespace {
constexpr int kLimbs = 9;  // fe29.h NL: limbs (planes) per value

struct DevBuf {
  void* p = nullptr;
  ~DevBuf() { if (p) (void)hipFree(p); }
  bool alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 4) == hipSuccess; }
  template <class T> T* as() { return static_cast<T*>(p); }
};
}  // namespace

extern "C" {

uint64_t table_check_entries(int wbits) { return mbft_launch::table_entries(wbits); }
uint64_t table_check_words(int wbits) { return mbft_launch::table_words(wbits); }
int table_check_steps(int wbits) { return mbft_launch::table_steps(wbits); }

// xy: npts x 16 LE words (plain affine x, y).  Builds the npts comb tables
// for window wbits (mbft_launch::build_tables) and copies back either every
// entry (idx null: out holds npts * table_entries * 16 words) or the nidx
// entries at the given global indices (out: nidx * 16 words).
int table_check_run(const uint32_t* xy, int npts, int wbits, const uint64_t* idx, long nidx,
                    uint32_t* out) {
  if (npts <= 0 || wbits < mbft_launch::kMinWindow || wbits > mbft_launch::kMaxWindow) return -1;
  const size_t ent = mbft_launch::table_entries(wbits);
  const size_t total = ent * (size_t)npts;
  if (idx)
    for (long k = 0; k < nidx; k++)
      if (idx[k] >= total) return -1;
  DevBuf d_xy, d_b, d_tab;
  if (!d_xy.alloc(64 * (size_t)npts) ||
      !d_b.alloc(64 * (size_t)npts * (size_t)mbft_launch::table_steps(wbits)) ||
      !d_tab.alloc(64 * total))
    return -2;
  if (hipMemcpy(d_xy.p, xy, 64 * (size_t)npts, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemset(d_tab.p, 0xEE, 64 * total) != hipSuccess)
    return -3;
  if (mbft_launch::build_tables(d_xy.as<uint32_t>(), npts, wbits, d_b.as<uint32_t>(),
                                d_tab.as<uint32_t>(), nullptr) != hipSuccess ||
      hipDeviceSynchronize() != hipSuccess)
    return -4;
  if (!idx)
    return hipMemcpy(out, d_tab.p, 64 * total, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -5;
  for (long k = 0; k < nidx; k++)
    if (hipMemcpy(out + 16 * k, d_tab.as<uint32_t>() + 16 * idx[k], 64, hipMemcpyDeviceToHost) !=
        hipSuccess)
      return -5;
  return 0;
}

// s: n x 32 big-endian bytes.  planes_out: 9 x n words, limb k of item i at
// k * n + i: the s^-1 planes of form 0 (the level chain, batch_inverse_s with
// a workspace of ninv_workspace_words(n)), 1 (batch_inverse_s_local) or 2
// (batch_inverse_s_pipelined).
int ninv_check_run(int form, const uint8_t* s, long n, uint32_t* planes_out) {
  if (n <= 0 || form < 0 || form > 2) return -1;
  DevBuf d_s, d_w, d_ws, d_zero;
  const size_t pbytes = 4 * (size_t)kLimbs * (size_t)n;
  if (!d_s.alloc(32 * (size_t)n) || !d_w.alloc(pbytes) || !d_zero.alloc(4) ||
      !d_ws.alloc(form == 0 ? 4 * mbft_launch::ninv_workspace_words(n) : 4))
    return -2;
  if (hipMemcpy(d_s.p, s, 32 * (size_t)n, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemset(d_w.p, 0xEE, pbytes) != hipSuccess || hipMemset(d_zero.p, 0xEE, 4) != hipSuccess)
    return -3;
  hipError_t e;
  if (form == 0)
    e = mbft_launch::batch_inverse_s(d_s.as<uint8_t>(), n, d_ws.as<uint32_t>(), d_w.as<uint32_t>(),
                                     d_zero.as<uint32_t>(), nullptr);
  else if (form == 1)
    e = mbft_launch::batch_inverse_s_local(d_s.as<uint8_t>(), n, d_w.as<uint32_t>(),
                                           d_zero.as<uint32_t>(), nullptr);
  else
    e = mbft_launch::batch_inverse_s_pipelined(d_s.as<uint8_t>(), n, d_w.as<uint32_t>(),
                                               d_zero.as<uint32_t>(), nullptr);
  if (e != hipSuccess || hipDeviceSynchronize() != hipSuccess) return -4;
  uint32_t zero = 1;
  if (hipMemcpy(planes_out, d_w.p, pbytes, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(&zero, d_zero.p, 4, hipMemcpyDeviceToHost) != hipSuccess)
    return -5;
  return zero == 0 ? 0 : -6;  // every form zeroes the word it is handed
}

// ---------------------------------------------------------------------------
// The large path on a caller-chosen grid (tests/test_gpu_verify_passes.py).

// the grid rules (verify_plan.h) and the device's compute units, so that the
// Python side counts a case's passes from the product's own rule
long verify_check_device_cus() { return mbft_launch::device_cus(); }
long verify_check_large_blocks(long blocks, long bpc, long ncu) { return mbft::verify_large_blocks(blocks, bpc, ncu); }
long verify_check_slow_blocks(long blocks, long vblocks, long ncu) {
  return mbft::verify_slow_blocks(blocks, vblocks, ncu);
}
long verify_check_ladder_blocks(long blocks, long ncu) { return mbft::verify_ladder_blocks(blocks, ncu); }
long verify_check_keys_blocks(long n, unsigned long lane_inv_max, long ncu) {
  return mbft::verify_keys_plan(n, (size_t)lane_inv_max, ncu).blocks;
}

// mbft_launch::verify's kLarge form (k_verify, k_verify_slow, k_verify_ladder)
// over n items on a grid of grid_blocks blocks (0: the plan's own), as
// MBFT_VERIFY_BPC caps it in the product.
// xy: npts x 16 LE words (plain affine x, y); cls: per point a comb window
// (kMinWindow ..), 0, kTeethFlag | t or kSignedTeethFlag | t; invalid: per
// point, 1 -> KeyDesc.valid = 0.  Point k is key slot k, its data built by the
// class's own builder.  e, r, s: n x 32 B big-endian; slot: n words; wg: the
// generator window.
// Out: status (n bytes); qlen: the exact queue's length word and the ladder
// queue's, as left in the buffer; slowq_out / ladderq_out: the n words of
// either queue (words no push reached still hold 0xEEEEEEEE); guards: bit 0
// the 256 bytes behind the statuses, 1 the words between the length words and
// the ladder queue, 2 those between the ladder queue and the spill planes, 3
// the 64 words behind the spill planes -- set where every byte is still 0xEE
// (the queues' places follow from n in the kernels, so their guard lines are
// the alignment gaps of the layout; a region may be empty).
int verify_check_run(const uint32_t* xy, const uint32_t* cls, const uint8_t* invalid, int npts,
                     const uint8_t* e, const uint8_t* r, const uint8_t* s, const uint32_t* slot, long n,
                     int wg, long grid_blocks, uint8_t* status, uint32_t* qlen, uint32_t* slowq_out,
                     uint32_t* ladderq_out, int* guards) {
  using mbft::KeyDesc;
  if (npts <= 0 || n <= 0 || grid_blocks < 0 || wg < mbft_launch::kMinWindow || wg > 16) return -1;
  // every key's data, class by class
  auto class_words = [](uint32_t c) -> size_t {
    if (c >= mbft::kSignedTeethFlag) return mbft_launch::steeth_table_words((int)(c & 0xFFu));
    if (c >= mbft::kTeethFlag) return mbft_launch::teeth_table_words((int)(c & 0xFFu));
    return c == 0u ? 16u : mbft_launch::table_words((int)c);
  };
  size_t total_words = 0;
  bool table_free = false;
  for (int k = 0; k < npts; k++) {
    const uint32_t c = cls[k], t = c & 0xFFu;
    const bool ok = c >= mbft::kSignedTeethFlag
                        ? (c == (mbft::kSignedTeethFlag | t) && (int)t >= mbft_launch::kSteethMin &&
                           (int)t <= mbft_launch::kSteethMax)
                        : c >= mbft::kTeethFlag ? ((int)t >= mbft_launch::kTeethMin && (int)t <= mbft_launch::kTeethMax)
                                                : (c == 0u || (c >= (uint32_t)mbft_launch::kMinWindow && c <= 12u));
    if (!ok) return -1;
    total_words += class_words(c);
    table_free = table_free || mbft::key_class_queued(c);
  }
  DevBuf d_gxy, d_gb, d_tabG, d_tabs, d_xy, d_b, d_keys;
  if (!d_gxy.alloc(64) || !d_gb.alloc(64 * (size_t)mbft_launch::table_steps(wg)) ||
      !d_tabG.alloc(4 * mbft_launch::table_words(wg)) || !d_tabs.alloc(4 * total_words) ||
      !d_xy.alloc(64 * (size_t)npts) || !d_keys.alloc(sizeof(KeyDesc) * (size_t)npts))
    return -2;
  if (mbft_launch::generator_xy(d_gxy.as<uint32_t>(), nullptr) != hipSuccess ||
      mbft_launch::build_tables(d_gxy.as<uint32_t>(), 1, wg, d_gb.as<uint32_t>(), d_tabG.as<uint32_t>(),
                                nullptr) != hipSuccess)
    return -4;
  KeyDesc* kd = new KeyDesc[npts];
  uint32_t* hxy = new uint32_t[16 * (size_t)npts];
  bool* done = new bool[npts]();
  struct Free {
    KeyDesc* a;
    uint32_t* b;
    bool* c;
    ~Free() { delete[] a; delete[] b; delete[] c; }
  } free_host{kd, hxy, done};
  uint32_t* next = d_tabs.as<uint32_t>();
  for (int first = 0; first < npts; first++) {
    if (done[first]) continue;
    const uint32_t c = cls[first];
    int cnt = 0;
    for (int k = first; k < npts; k++)
      if (cls[k] == c) {
        for (int j = 0; j < 16; j++) hxy[16 * (size_t)cnt + j] = xy[16 * (size_t)k + j];
        kd[k] = KeyDesc{next + class_words(c) * (size_t)cnt, c, invalid[k] ? 0u : 1u};
        done[k] = true;
        cnt++;
      }
    if (hipMemcpy(d_xy.p, hxy, 64 * (size_t)cnt, hipMemcpyHostToDevice) != hipSuccess) return -3;
    hipError_t be;
    if (c >= mbft::kSignedTeethFlag) {
      be = mbft_launch::build_steeth_tables(d_xy.as<uint32_t>(), cnt, (int)(c & 0xFFu), next, nullptr);
    } else if (c >= mbft::kTeethFlag) {
      be = mbft_launch::build_teeth_tables(d_xy.as<uint32_t>(), cnt, (int)(c & 0xFFu), next, nullptr);
    } else if (c == 0u) {
      be = mbft_launch::point_entries(d_xy.as<uint32_t>(), cnt, next, nullptr);
    } else {
      DevBuf d_kb;
      if (!d_kb.alloc(64 * (size_t)cnt * (size_t)mbft_launch::table_steps((int)c))) return -2;
      be = mbft_launch::build_tables(d_xy.as<uint32_t>(), cnt, (int)c, d_kb.as<uint32_t>(), next, nullptr);
      if (hipDeviceSynchronize() != hipSuccess) return -4;  // (d_kb is read until the build ends)
    }
    if (be != hipSuccess || hipDeviceSynchronize() != hipSuccess) return -4;
    next += class_words(c) * (size_t)cnt;
  }
  if (hipMemcpy(d_keys.p, kd, sizeof(KeyDesc) * (size_t)npts, hipMemcpyHostToDevice) != hipSuccess) return -3;

  // the plan: the large form, on the caller's grid
  mbft::VerifyPlan plan = mbft::verify_plan(n, mbft::InvSource::kBatch, false, true, 0, 0);
  if (plan.form != mbft::VerifyForm::kLarge || plan.threads != n) return -7;
  if (grid_blocks > 0) plan.threads = 256 * grid_blocks;
  const size_t qwords = mbft::verify_slowq_words(n, plan), lq = mbft::ladder_queue_offset(n),
               so = mbft::verify_scratch_offset(n);
  constexpr size_t kStatusGuard = 256, kTailGuard = 64;
  DevBuf d_e, d_r, d_s, d_slot, d_st, d_q, d_w;
  if (!d_e.alloc(32 * (size_t)n) || !d_r.alloc(32 * (size_t)n) || !d_s.alloc(32 * (size_t)n) ||
      !d_slot.alloc(4 * (size_t)n) || !d_st.alloc((size_t)n + kStatusGuard) ||
      !d_q.alloc(4 * (qwords + kTailGuard)) || !d_w.alloc(4 * (size_t)kLimbs * (size_t)n))
    return -2;
  if (hipMemcpy(d_e.p, e, 32 * (size_t)n, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(d_r.p, r, 32 * (size_t)n, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(d_s.p, s, 32 * (size_t)n, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(d_slot.p, slot, 4 * (size_t)n, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemset(d_st.p, 0xEE, (size_t)n + kStatusGuard) != hipSuccess ||
      hipMemset(d_q.p, 0xEE, 4 * (qwords + kTailGuard)) != hipSuccess ||
      hipDeviceSynchronize() != hipSuccess)
    return -3;
  // s^-1 as the product runs it on an idle engine: the exact queue's length
  // word is zeroed by the same kernel
  if (mbft_launch::batch_inverse_s_local(d_s.as<uint8_t>(), n, d_w.as<uint32_t>(), d_q.as<uint32_t>() + n,
                                         nullptr) != hipSuccess)
    return -4;
  const mbft_launch::VerifyBatch vb{d_e.as<uint8_t>(), d_r.as<uint8_t>(), d_s.as<uint8_t>(), d_slot.as<uint32_t>(),
                                    n, d_st.as<uint8_t>(), d_q.as<uint32_t>(), d_w.as<uint32_t>(), nullptr, nullptr,
                                    false};
  const mbft_launch::VerifyTables vt{d_tabG.as<uint32_t>(), wg, d_keys.as<KeyDesc>(), (uint32_t)npts, table_free};
  if (mbft_launch::verify(vb, vt, plan, nullptr) != hipSuccess || hipDeviceSynchronize() != hipSuccess) return -4;

  uint8_t* hst = new uint8_t[(size_t)n + kStatusGuard];
  uint32_t* hq = new uint32_t[qwords + kTailGuard];
  struct Free2 {
    uint8_t* a;
    uint32_t* b;
    ~Free2() { delete[] a; delete[] b; }
  } free_out{hst, hq};
  if (hipMemcpy(hst, d_st.p, (size_t)n + kStatusGuard, hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(hq, d_q.p, 4 * (qwords + kTailGuard), hipMemcpyDeviceToHost) != hipSuccess)
    return -5;
  auto clean = [&](size_t from, size_t to) {
    for (size_t k = from; k < to; k++)
      if (hq[k] != 0xEEEEEEEEu) return false;
    return true;
  };
  int g = 1;
  for (size_t k = 0; k < kStatusGuard; k++)
    if (hst[(size_t)n + k] != 0xEE) g = 0;
  if (clean((size_t)n + 2, lq)) g |= 2;
  if (clean(lq + (size_t)n, so)) g |= 4;
  if (clean(qwords, qwords + kTailGuard)) g |= 8;
  *guards = g;
  for (long k = 0; k < n; k++) {
    status[k] = hst[k];
    slowq_out[k] = hq[k];
    ladderq_out[k] = hq[lq + (size_t)k];
  }
  qlen[0] = hq[n];
  qlen[1] = hq[n + 1];
  return 0;
}

// mbft_launch::verify_keys (k_verify_keys) over n items on a grid of `blocks`
// blocks: xy n x 64 B big-endian X || Y, lane_inv as KeysPlan's (0: s^-1 from
// the planes of batch_inverse_s_local).  Out: status (n bytes); *guard: 1 where
// the 256 bytes behind the statuses are still 0xEE.
int verify_keys_check_run(const uint8_t* e, const uint8_t* r, const uint8_t* s, const uint8_t* xy, long n, int wg,
                          long blocks, int lane_inv, uint8_t* status, int* guard) {
  if (n <= 0 || blocks <= 0 || wg < mbft_launch::kMinWindow || wg > 16) return -1;
  constexpr size_t kStatusGuard = 256;
  DevBuf d_gxy, d_gb, d_tabG, d_e, d_r, d_s, d_xy, d_st, d_w;
  if (!d_gxy.alloc(64) || !d_gb.alloc(64 * (size_t)mbft_launch::table_steps(wg)) ||
      !d_tabG.alloc(4 * mbft_launch::table_words(wg)) || !d_e.alloc(32 * (size_t)n) || !d_r.alloc(32 * (size_t)n) ||
      !d_s.alloc(32 * (size_t)n) || !d_xy.alloc(64 * (size_t)n) || !d_st.alloc((size_t)n + kStatusGuard) ||
      !d_w.alloc(4 * (size_t)kLimbs * (size_t)n))
    return -2;
  if (mbft_launch::generator_xy(d_gxy.as<uint32_t>(), nullptr) != hipSuccess ||
      mbft_launch::build_tables(d_gxy.as<uint32_t>(), 1, wg, d_gb.as<uint32_t>(), d_tabG.as<uint32_t>(),
                                nullptr) != hipSuccess)
    return -4;
  if (hipMemcpy(d_e.p, e, 32 * (size_t)n, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(d_r.p, r, 32 * (size_t)n, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(d_s.p, s, 32 * (size_t)n, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemcpy(d_xy.p, xy, 64 * (size_t)n, hipMemcpyHostToDevice) != hipSuccess ||
      hipMemset(d_st.p, 0xEE, (size_t)n + kStatusGuard) != hipSuccess || hipDeviceSynchronize() != hipSuccess)
    return -3;
  if (!lane_inv && mbft_launch::batch_inverse_s_local(d_s.as<uint8_t>(), n, d_w.as<uint32_t>(), nullptr, nullptr) !=
                       hipSuccess)
    return -4;
  const mbft_launch::KeysBatch kb{d_e.as<uint8_t>(), d_r.as<uint8_t>(), d_s.as<uint8_t>(), d_xy.as<uint8_t>(), n,
                                  d_st.as<uint8_t>(), lane_inv ? nullptr : d_w.as<uint32_t>()};
  const mbft::KeysPlan plan{lane_inv != 0, (n + 255) / 256 * 256, blocks};
  if (mbft_launch::verify_keys(kb, d_tabG.as<uint32_t>(), wg, plan, nullptr) != hipSuccess ||
      hipDeviceSynchronize() != hipSuccess)
    return -4;
  uint8_t* hst = new uint8_t[(size_t)n + kStatusGuard];
  const bool ok = hipMemcpy(hst, d_st.p, (size_t)n + kStatusGuard, hipMemcpyDeviceToHost) == hipSuccess;
  int g = 1;
  for (size_t k = 0; ok && k < kStatusGuard; k++)
    if (hst[(size_t)n + k] != 0xEE) g = 0;
  for (long k = 0; ok && k < n; k++) status[k] = hst[k];
  delete[] hst;
  *guard = g;
  return ok ? 0 : -5;
}

}  // extern "C"
