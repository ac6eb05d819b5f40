// Test-only harness (tests/test_gpu_arena_dev.py, tests/test_gpu_msg_dedup.py,
// tests/test_gpu_msg_number.py, tests/test_gpu_msg_replay.py): runs the device
// message layer stage by stage
// through the library's own launchers (minbft_amd/csrc/msg_dev.h, linked from
// libminbft_amd.so) over a fabricated MsgDevArgs -- no context -- and hands
// every intermediate array back, so that Python can check each stage against
// a model and can INJECT state no honest run produces on demand: candidates
// with equal content hashes and different content (stage_run's forcing),
// numbering inputs of any shape (number_run), uploads of any length
// (upload_run), checks, call outcomes and epoch state of any shape for the
// optimistic replay (replay_run).  arena_run calls the blocked arena reads of arena_dev.h,
// included directly, one case per lane.  The functions are the product's own,
// called, not restated.  Every entry point checks its arguments before the
// first launch (fields inside the arena, indices in range, table capacity),
// checks every HIP call, returns at the first failure and launches nothing
// after it.  Built into tests/libmsg_stage_check.so by
// __graft_entry__.build(); never part of the product library.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../minbft_amd/csrc/arena_dev.h"
#include "../../minbft_amd/csrc/msg_dev.h"

using namespace mbft;

namespace {

constexpr int kMark = 0xAA;  // every output byte before the launches
constexpr long kMaxMsgs = 1L << 20;

// Device buffers, one page-locked host buffer and one stream around a run;
// ok stays false after the first HIP call that fails.
struct Run {
  std::vector<void*> dev;
  void* host = nullptr;
  hipStream_t st = nullptr;
  bool ok = true;
  ~Run() {
    for (void* p : dev) (void)hipFree(p);
    if (host) (void)hipHostFree(host);
    if (st) (void)hipStreamDestroy(st);
  }
  bool stream() {
    if (ok && hipStreamCreate(&st) != hipSuccess) ok = false;
    return ok;
  }
  void* raw(size_t bytes) {
    void* d = nullptr;
    if (!ok || hipMalloc(&d, bytes ? bytes : 4) != hipSuccess) {
      ok = false;
      return nullptr;
    }
    dev.push_back(d);
    return d;
  }
  template <class T> T* in(const T* h, size_t count) {
    T* d = static_cast<T*>(raw(sizeof(T) * count));
    if (d && count && hipMemcpy(d, h, sizeof(T) * count, hipMemcpyHostToDevice) != hipSuccess) ok = false;
    return d;
  }
  template <class T> T* out(size_t count) {
    T* d = static_cast<T*>(raw(sizeof(T) * count));
    if (d && hipMemset(d, kMark, sizeof(T) * (count ? count : 1)) != hipSuccess) ok = false;
    return d;
  }
  template <class T> void up(T* d, const T* h, size_t count) {
    if (ok && count && hipMemcpy(d, h, sizeof(T) * count, hipMemcpyHostToDevice) != hipSuccess) ok = false;
  }
  template <class T> void back(T* h, const T* d, size_t count) {
    if (ok && count && hipMemcpy(h, d, sizeof(T) * count, hipMemcpyDeviceToHost) != hipSuccess) ok = false;
  }
  // the arena as the product allocates it (msgdev.cpp: ((nbytes + 3) & ~3) + 32,
  // the padding zeroed)
  uint8_t* arena(const uint8_t* h, uint64_t nbytes) {
    const size_t size = (((size_t)nbytes + 3) & ~(size_t)3) + 32;
    uint8_t* d = static_cast<uint8_t*>(raw(size));
    if (d && hipMemset(d, 0, size) != hipSuccess) ok = false;
    if (d) up(d, h, (size_t)nbytes);
    return d;
  }
  void launched(hipError_t e) {
    if (e != hipSuccess) ok = false;
  }
  void sync() {
    if (ok && (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess)) ok = false;
  }
};

bool field_in(uint64_t off, uint32_t len, uint64_t nbytes) {
  return len == 0 || (off <= nbytes && (uint64_t)len <= nbytes - off);
}

bool table_cap_ok(uint32_t cap, long n) {
  return cap >= 4 && (cap & (cap - 1)) == 0 && (uint64_t)cap >= 2ull * 3ull * (uint64_t)n;
}

// the dedup table's home slot of a hash (msg_kernels.hip dedup_insert)
uint32_t home_slot(uint64_t h, uint32_t tmask) { return (uint32_t)(h ^ (h >> 29)) & tmask; }

// scan + base + call list, or the single-workgroup form; *rc = the numbering
// launcher's own return value
void number(Run& R, const MsgDevArgs& a, long n, uint32_t* bounds, bool one, hipError_t* rc) {
  if (!R.ok) return;
  if (one) {
    *rc = mbft_launch::msg_number_one(a, 0, n, bounds, 0, R.st);
    return;
  }
  size_t tmp_bytes = 0;
  *rc = mbft_launch::msg_scan(a, 0, 0, n + 1, nullptr, &tmp_bytes, R.st);
  if (*rc != hipSuccess) return;
  void* tmp = R.raw(tmp_bytes + 16);
  if (!R.ok) return;
  *rc = mbft_launch::msg_scan(a, 0, n, 0, tmp, &tmp_bytes, R.st);
  if (*rc != hipSuccess) return;
  *rc = mbft_launch::msg_number(a, 0, n, bounds, 0, R.st);
}

}  // namespace

// op 0: sha256_arena(off, len) -> 8 words (big-endian-numeric, as the kernels
// use them); op 1: arena_block(arena_field(off, len), k0) -> 8 words; op 2:
// stage_field(off, len) into the lane's LDS slot (pre-filled with the marker)
// -> the return value, then the slot's 25 words.
__global__ void __launch_bounds__(64) k_arena(int op, const uint8_t* b, const uint64_t* off, const uint32_t* len,
                                              const uint32_t* k0, uint32_t* out, int n) {
  __shared__ uint32_t lds[64 * kTagWords];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (op == 0) {
    uint32_t h[8];
    sha256_arena(h, b, off[i], len[i]);
    for (int j = 0; j < 8; j++) out[(size_t)8 * i + j] = h[j];
  } else if (op == 1) {
    const ArenaField f = arena_field(b, off[i], len[i]);
    uint32_t o[8];
    arena_block(f, k0[i], o);
    for (int j = 0; j < 8; j++) out[(size_t)8 * i + j] = o[j];
  } else {
    uint32_t* slot = lds + threadIdx.x * kTagWords;
    for (int j = 0; j < kTagWords; j++) slot[j] = 0x01010101u * (uint32_t)kMark;
    const bool ok = stage_field(slot, b, off[i], len[i]);
    out[(size_t)(kTagWords + 1) * i] = ok ? 1u : 0u;
    for (int j = 0; j < kTagWords; j++) out[(size_t)(kTagWords + 1) * i + 1 + j] = slot[j];
  }
}

extern "C" {

long msg_stage_number_one_max() { return mbft_launch::kNumberOneMax; }
int msg_stage_tag_words() { return kTagWords; }
int msg_stage_cand_size() { return (int)sizeof(MsgCand); }
int msg_stage_info_size() { return (int)sizeof(DevCallInfo); }
int msg_stage_rec_size() { return (int)sizeof(mbft_msg_rec); }

// n cases over one arena; out: 8 words per case (op 0, 1) or 26 (op 2).
// Every non-empty field must lie inside the arena; arena_block needs len > 0
// (an empty field has no covering word).
int arena_run(int op, const uint8_t* arena, uint64_t nbytes, const uint64_t* off, const uint32_t* len,
              const uint32_t* k0, int n, uint32_t* out) {
  if (op < 0 || op > 2 || n <= 0 || n > (1 << 20) || nbytes > (1ull << 30)) return -1;
  for (int i = 0; i < n; i++)
    if (!field_in(off[i], len[i], nbytes) || (op == 1 && len[i] == 0)) return -1;
  const size_t per = op == 2 ? kTagWords + 1 : 8;
  Run R;
  uint8_t* d_b = R.arena(arena, nbytes);
  uint64_t* d_off = R.in(off, n);
  uint32_t* d_len = R.in(len, n);
  uint32_t* d_k0 = R.in(k0, n);
  uint32_t* d_out = R.out<uint32_t>(per * n);
  if (!R.stream()) return -2;
  hipLaunchKernelGGL(k_arena, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, R.st, op, d_b, d_off, d_len, d_k0,
                     d_out, n);
  R.sync();
  if (!R.ok) return -4;
  R.back(out, d_out, per * n);
  return R.ok ? 0 : -5;
}

// The device message layer over n records and their arena, stage by stage on
// one stream: msg_init -> msg_cands -> (forcing) -> msg_dedup_resolve ->
// numbering (number_one: msg_number_one, else msg_scan + msg_number + the
// call list) -> msg_calls.
//   km_key / km_slot (nk pairs): the key map's contents, (role << 32) | id ->
//     key slot; the map is built here with keymap_hash (empty = ~0, capacity a
//     power of two at load <= 1/2).  key_valid / fpg: per key slot (nslots).
//   group (optional, 3n): after msg_cands has completed, every candidate with
//     chash != 0 and group[c] != 0 gets group[c] as its hash (0 keeps the
//     honest hash), and tkeys / treps / cslot are rebuilt on the host by
//     dedup_insert's rule -- one slot per distinct hash, the slot keeps the
//     smallest candidate index -- exactly the state an honest run leaves when
//     those hashes collide.
// Outputs (3n entries each unless noted; what no kernel writes keeps the 0xAA
// marker): bad (1), chk (n), cand, chash, uniq, ref, idx, call_of, cand_of,
// bounds (2), and per unique call e, r, s (32 B each), slot, info.
int stage_run(const mbft_msg_rec* recs, long n, const uint8_t* arena, uint64_t nbytes, uint32_t n_replicas,
              uint32_t cap, const uint64_t* km_key, const uint32_t* km_slot, uint32_t nk, uint32_t role_ok,
              const uint32_t* key_valid, const uint32_t* fpg, uint32_t nslots, const uint64_t* group,
              int number_one, uint32_t* bad, uint32_t* chk, MsgCand* cand, uint64_t* chash, uint32_t* uniq,
              uint32_t* ref, uint32_t* idx, uint32_t* call_of, uint32_t* cand_of, uint32_t* bounds, uint8_t* e,
              uint8_t* r, uint8_t* s, uint32_t* slot, DevCallInfo* info) {
  if (n <= 0 || n > kMaxMsgs || n_replicas == 0 || nbytes > (1ull << 30) || nk > (1u << 20) ||
      nslots > (1u << 20) || !table_cap_ok(cap, n))
    return -1;
  if (number_one && 3 * n > mbft_launch::kNumberOneMax) return -1;
  for (long i = 0; i < n; i++) {
    const mbft_msg_rec& m = recs[i];
    if (!field_in(m.op_off, m.op_len, nbytes) || !field_in(m.sig_off, m.sig_len, nbytes) ||
        !field_in(m.ui_cert_off, m.ui_cert_len, nbytes) ||
        !field_in(m.prep_ui_cert_off, m.prep_ui_cert_len, nbytes))
      return -1;
  }
  // the key map
  uint32_t kcap = 4;
  while (kcap < 2 * nk) kcap <<= 1;
  std::vector<uint64_t> mk(kcap, ~0ull);
  std::vector<uint32_t> ms(kcap, 0);
  for (uint32_t j = 0; j < nk; j++) {
    if (km_key[j] == ~0ull) return -1;
    uint32_t h = keymap_hash(km_key[j]) & (kcap - 1);
    while (mk[h] != ~0ull && mk[h] != km_key[j]) h = (h + 1) & (kcap - 1);
    if (mk[h] == km_key[j]) return -1;  // one slot per key
    mk[h] = km_key[j];
    ms[h] = km_slot[j];
  }
  std::vector<KeyDesc> kd(nslots ? nslots : 1, KeyDesc{nullptr, 0, 0});
  for (uint32_t j = 0; j < nslots; j++) kd[j].valid = key_valid[j];

  const size_t nc3 = 3 * (size_t)n;
  Run R;
  MsgDevArgs a{};
  a.recs = R.in(recs, n);
  a.bytes = R.arena(arena, nbytes);
  a.nbytes = nbytes;
  a.n = n;
  a.n_replicas = n_replicas;
  uint32_t* flags = R.out<uint32_t>(16);
  uint32_t* d_bounds = R.out<uint32_t>(16);
  a.bad = flags;
  a.chk = R.out<uint32_t>(n);
  a.cand = R.out<MsgCand>(nc3);
  a.chash = R.out<uint64_t>(nc3);
  a.cslot = R.out<uint32_t>(nc3);
  a.uniq = R.out<uint32_t>(nc3);
  a.ref = R.out<uint32_t>(nc3);
  a.idx = R.out<uint32_t>(nc3);
  a.call_of = R.out<uint32_t>(nc3);
  a.cand_of = R.out<uint32_t>(nc3);
  a.tkeys = R.out<unsigned long long>(cap);
  a.treps = R.out<uint32_t>(cap);
  a.tmask = cap - 1;
  a.map = KeyMap{R.in(mk.data(), kcap), R.in(ms.data(), kcap), kcap - 1, role_ok};
  a.keys = R.in(kd.data(), kd.size());
  a.nslots = nslots;
  a.fpg = R.in(fpg, nslots);
  a.e = R.out<uint8_t>(32 * nc3 + 32);
  a.r = R.out<uint8_t>(32 * nc3 + 32);
  a.s = R.out<uint8_t>(32 * nc3 + 32);
  a.slot = R.out<uint32_t>(nc3 + 1);
  a.info = R.out<DevCallInfo>(nc3 + 2);
  if (!R.stream()) return -2;

  R.launched(mbft_launch::msg_init(a, flags, d_bounds, R.st));
  if (R.ok) R.launched(mbft_launch::msg_cands(a, 0, n, R.st));
  R.sync();
  if (!R.ok) return -4;
  if (group) {
    std::vector<uint64_t> h(nc3);
    R.back(h.data(), a.chash, nc3);
    if (!R.ok) return -5;
    std::vector<unsigned long long> tk(cap, 0ull);
    std::vector<uint32_t> tr(cap, ~0u), cs(nc3, 0);
    for (size_t c = 0; c < nc3; c++) {
      if (h[c] == 0) continue;
      if (group[c] != 0) h[c] = group[c];
      uint32_t sl = home_slot(h[c], a.tmask);
      while (tk[sl] != 0ull && tk[sl] != h[c]) sl = (sl + 1) & a.tmask;  // load <= 1/2: ends
      if (tk[sl] == 0ull) {
        tk[sl] = h[c];
        tr[sl] = (uint32_t)c;  // ascending c: the first is the smallest
      }
      cs[c] = sl;
    }
    R.up(a.chash, h.data(), nc3);
    R.up(a.tkeys, tk.data(), cap);
    R.up(a.treps, tr.data(), cap);
    R.up(a.cslot, cs.data(), nc3);
    if (!R.ok) return -3;
  }
  R.launched(mbft_launch::msg_dedup_resolve(a, 0, n, R.st));
  hipError_t nrc = hipSuccess;
  number(R, a, n, d_bounds, number_one != 0, &nrc);
  R.launched(nrc);
  if (R.ok)
    R.launched(mbft_launch::msg_calls(a, 0, n, 0, (long)nc3, R.st, d_bounds + 1, number_one != 0));
  R.sync();
  if (!R.ok) return -4;
  R.back(bad, flags, 1);
  R.back(chk, a.chk, n);
  R.back(cand, a.cand, nc3);
  R.back(chash, a.chash, nc3);
  R.back(uniq, a.uniq, nc3);
  R.back(ref, a.ref, nc3);
  R.back(idx, a.idx, nc3);
  R.back(call_of, a.call_of, nc3);
  R.back(cand_of, a.cand_of, nc3);
  R.back(bounds, d_bounds, 2);
  R.back(e, a.e, 32 * nc3);
  R.back(r, a.r, 32 * nc3);
  R.back(s, a.s, 32 * nc3);
  R.back(slot, a.slot, nc3);
  R.back(info, a.info, nc3);
  return R.ok ? 0 : -5;
}

// The numbering alone over injected state for the 3n slots of n messages:
// chash (only zero / not zero matters), uniq (0 / 1), ref (< 3n), and the
// running base bounds[0].  one: msg_number_one; else msg_scan + msg_number +
// the call list (msg_calls with no call to decode).  *launch_rc = the
// numbering launcher's return value (msg_number_one refuses 3n >
// kNumberOneMax and launches nothing: the outputs keep the marker).
// Outputs: idx, call_of (3n), cand_of (bounds0 + 3n: call k's slot is
// absolute), bounds1.
int number_run(long n, const uint64_t* chash, const uint32_t* uniq, const uint32_t* ref, uint32_t bounds0,
               int one, uint32_t* idx, uint32_t* call_of, uint32_t* cand_of, uint32_t* bounds1,
               int* launch_rc) {
  if (n <= 0 || n > kMaxMsgs || bounds0 > (1u << 20)) return -1;
  const size_t nc3 = 3 * (size_t)n;
  for (size_t c = 0; c < nc3; c++)
    if (uniq[c] > 1u || ref[c] >= nc3) return -1;
  Run R;
  MsgDevArgs a{};
  a.n = n;
  a.chash = R.in(const_cast<uint64_t*>(chash), nc3);
  a.uniq = R.in(const_cast<uint32_t*>(uniq), nc3);
  a.ref = R.in(const_cast<uint32_t*>(ref), nc3);
  a.idx = R.out<uint32_t>(nc3);
  a.call_of = R.out<uint32_t>(nc3);
  a.cand_of = R.out<uint32_t>(bounds0 + nc3);
  uint32_t* d_bounds = R.out<uint32_t>(16);
  R.up(d_bounds, &bounds0, 1);
  if (!R.stream()) return -2;
  hipError_t nrc = hipSuccess;
  number(R, a, n, d_bounds, one != 0, &nrc);
  *launch_rc = (int)nrc;
  if (R.ok && nrc == hipSuccess && !one) R.launched(mbft_launch::msg_calls(a, 0, n, 0, 0, R.st));
  R.sync();
  if (!R.ok) return -4;
  R.back(idx, a.idx, nc3);
  R.back(call_of, a.call_of, nc3);
  R.back(cand_of, a.cand_of, bounds0 + nc3);
  R.back(bounds1, d_bounds + 1, 1);
  return R.ok ? 0 : -5;
}

// k_msg_init's in-kernel upload: `bytes` bytes of src go to page-locked host
// memory (16-B aligned; the rest of its last 16-B chunk is 0xFF, which the
// upload must not carry over), the destination holds the marker, msg_init
// runs with MsgUpload{dst, src, bytes, fill}; out: the destination's first
// fill + 64 bytes.  fill: a multiple of 4, >= bytes, within the 16 tail words.
int upload_run(const uint8_t* src, uint64_t bytes, uint64_t fill, uint8_t* out) {
  if (bytes > (4ull << 20) || fill % 4 != 0 || fill < bytes || fill > (bytes & ~15ull) + 64) return -1;
  const size_t hsize = (((size_t)bytes + 15) & ~(size_t)15) + 16;
  const uint32_t cap = 1024;
  Run R;
  if (hipHostMalloc(&R.host, hsize, hipHostMallocDefault) != hipSuccess) return -2;
  if (((uintptr_t)R.host & 15u) != 0) return -2;
  memset(R.host, 0xFF, hsize);
  if (bytes) memcpy(R.host, src, (size_t)bytes);
  MsgDevArgs a{};
  a.tkeys = R.out<unsigned long long>(cap);
  a.treps = R.out<uint32_t>(cap);
  a.tmask = cap - 1;
  uint32_t* flags = R.out<uint32_t>(16);
  uint32_t* d_bounds = R.out<uint32_t>(16);
  uint8_t* dst = R.out<uint8_t>((size_t)fill + 64);
  if (!R.stream()) return -2;
  if (((uintptr_t)dst & 15u) != 0) return -2;
  const MsgUpload u{dst, static_cast<const uint8_t*>(R.host), bytes, fill};
  R.launched(mbft_launch::msg_init(a, flags, d_bounds, R.st, nullptr, &u, nullptr));
  R.sync();
  if (!R.ok) return -4;
  R.back(out, dst, (size_t)fill + 64);
  return R.ok ? 0 : -5;
}

// The optimistic replay alone (mbft_launch::msg_replay: k_replay_caps,
// k_replay_cap_epoch, k_replay_eval) over injected state: the packed checks
// of n messages, call_of for their 3n candidate slots, nc unique calls'
// outcomes (info, status) and the epoch state of G fingerprint groups.
//   out (out_len >= n + 8 words) and cap (cap_len >= 2G + 1 + 8 words; laid
//   out as msgdev.cpp lays it out: [0, G) cap_pos, [G, 2G) cap_epoch, [2G]
//   first_bad) are IN/OUT: uploaded whole as the caller filled them (cap_pos
//   ~0 and first_bad n, as msgdev.cpp does; sentinels behind), copied back
//   whole after the launch.
// Checked before anything is launched: every check count <= 3, every
// call_of < nc (all 3n: a check's slot comes from its byte, 0..2; slot 3
// refused; no call check without a call), every USIG call's fpg < G,
// epoch_set 0 / 1.  *launch_rc = the
// launcher's own return value (n == 0: success, nothing launched).
int replay_run(long n, const uint32_t* chk, const uint32_t* call_of, const DevCallInfo* info,
               const uint8_t* status, uint32_t nc, uint32_t G, const uint8_t* epoch_set,
               const uint64_t* epoch_val, int32_t* out, uint64_t out_len, uint64_t* cap, uint64_t cap_len,
               int* launch_rc) {
  if (n < 0 || n > kMaxMsgs || nc > 3u * (uint32_t)kMaxMsgs || G > (1u << 20) ||
      out_len < (uint64_t)n + 8 || out_len > (uint64_t)n + 4096 || cap_len < 2ull * G + 1 + 8 ||
      cap_len > 2ull * G + 1 + 4096)
    return -1;
  const size_t nc3 = 3 * (size_t)n;
  for (long i = 0; i < n; i++) {
    const uint32_t w = chk[i], nq = w & 0xFFu;
    if (nq > 3) return -1;
    for (uint32_t q = 0; q < nq; q++) {
      const uint32_t b = (w >> (8 + 8 * q)) & 0xFFu;
      if ((b & 3u) == kChkCall && (nc == 0 || ((b >> 6) & 3u) > 2u)) return -1;
    }
  }
  for (size_t c = 0; c < nc3; c++)
    if (nc != 0 && call_of[c] >= nc) return -1;
  for (uint32_t k = 0; k < nc; k++)
    if (info[k].usig > 1 || (info[k].usig && info[k].fpg >= G)) return -1;
  for (uint32_t g = 0; g < G; g++)
    if (epoch_set[g] > 1) return -1;
  Run R;
  MsgDevArgs a{};
  a.n = n;
  a.chk = R.in(chk, (size_t)n);
  a.call_of = R.in(call_of, nc3);
  a.info = R.in(info, nc);
  a.status = R.in(status, nc);
  a.epoch_set = R.in(epoch_set, G);
  a.epoch_val = R.in(epoch_val, G);
  a.ngroups = G;
  uint64_t* d_cap = R.in(cap, (size_t)cap_len);
  a.cap_pos = reinterpret_cast<unsigned long long*>(d_cap);
  a.cap_epoch = d_cap + G;
  a.first_bad = reinterpret_cast<unsigned long long*>(d_cap) + 2 * (size_t)G;
  a.out = R.in(out, (size_t)out_len);
  if (!R.stream()) return -2;
  const hipError_t rc = mbft_launch::msg_replay(a, R.st);
  *launch_rc = (int)rc;
  R.launched(rc);
  R.sync();
  if (!R.ok) return -4;
  R.back(out, a.out, (size_t)out_len);
  R.back(cap, d_cap, (size_t)cap_len);
  return R.ok ? 0 : -5;
}

}  // extern "C"
