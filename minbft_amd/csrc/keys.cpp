// The life of a key after registration: per-key use counts,
// re-classing of registered keys by hand and by count, removal with reuse of
// slot numbers and storage.  The decisions (free lists, the promotion choice)
// are key_plan.h's; registration itself is host.cpp's.  Every entry point that
// changes the key store holds KeyWriteGuard and replays the operation on the
// peer engines in the same order, so slot numbers and classes keep agreeing.
#include <algorithm>

#include "host_internal.h"

namespace mbft_host {

// The table engines of a context: its own, then the peers'.
static std::vector<mbft_ctx*> engines_of(mbft_ctx* c) {
  std::vector<mbft_ctx*> e{c};
  e.insert(e.end(), c->peers.begin(), c->peers.end());
  return e;
}

// Everything that may still read old key data or add to the counters has
// finished on the current device: the library's own batches are over
// (KeyWriteGuard), the caller-stream entry points return before their kernels
// do -- as mbft_clear_keys, the resident kernel parked first (the primary
// engine has it), then the whole device.
static int quiesce(mbft_ctx* c, mbft_ctx* e) {
  if (e == c) resident_park(c);
  HIPCHK(c, hipDeviceSynchronize());
  return MBFT_OK;
}

// The counters follow the slots: grown (x1.5 at least) and zero-filled, the
// counts so far carried over.  The adds of batches still in flight on caller
// streams must land before the copy: the device is synchronized (growth only).
int grow_key_counters(mbft_ctx* c) {
  const size_t ns = c->keydesc.size();
  if (c->d_uses && ns <= c->acct_slots) return MBFT_OK;
  size_t cap = ns < 1024 ? 1024 : ns;
  if (cap < c->acct_slots + c->acct_slots / 2) cap = c->acct_slots + c->acct_slots / 2;
  uint64_t* nu = nullptr;
  uint64_t* nr = nullptr;
  if (hipMalloc(&nu, cap * sizeof(uint64_t)) != hipSuccess || hipMalloc(&nr, cap * sizeof(uint64_t)) != hipSuccess) {
    (void)hipGetLastError();
    if (nu) (void)hipFree(nu);
    return fail(c, MBFT_ERR_NOMEM, "key use counts: out of device memory");
  }
  HIPCHK(c, hipMemsetAsync(nu, 0, cap * sizeof(uint64_t), c->stream));
  HIPCHK(c, hipMemsetAsync(nr, 0, cap * sizeof(uint64_t), c->stream));
  if (c->d_uses) {
    if (c->res) resident_park(c);
    HIPCHK(c, hipDeviceSynchronize());
    HIPCHK(c, hipMemcpyAsync(nu, c->d_uses, c->acct_slots * sizeof(uint64_t), hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(nr, c->d_rejects, c->acct_slots * sizeof(uint64_t), hipMemcpyDeviceToDevice, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (c->d_uses) (void)hipFree(c->d_uses);
  if (c->d_rejects) (void)hipFree(c->d_rejects);
  c->d_uses = nu;
  c->d_rejects = nr;
  c->acct_slots = cap;
  return MBFT_OK;
}

// ------------------------------------------------------ the verified-call memo
// (the shape and the rotation rule are memo_plan.h's.)

// The clear a quiet memo was asked for (M.m held, inflight == 0, the memo's
// device current): both generations where a clear is wanted, else the old one,
// which then becomes the young.  The memset goes on st with ev_clear behind
// it; the flags are lifted only where both were queued.  Returns the HIP
// error where they were not: the flags stay and passes go on without the memo.
static hipError_t memo_clear_quiet(VerifiedMemo& M, hipStream_t st) {
  const size_t gen_bytes = (size_t)M.rot.entries * mbft::kMemoEntryBytes;
  // (an earlier clear, on another stream, ends first: what follows this one is behind both)
  hipError_t e = M.ev_pending ? hipStreamWaitEvent(st, M.ev_clear, 0) : hipSuccess;
  if (e != hipSuccess) {
  } else if (M.clear_wanted) {
    e = hipMemsetAsync(M.tab, 0, 2 * gen_bytes, st);
  } else {
    const int old = M.rot.young ^ 1;
    e = hipMemsetAsync(reinterpret_cast<uint8_t*>(M.tab) + (size_t)old * gen_bytes, 0, gen_bytes, st);
  }
  if (e == hipSuccess) e = hipEventRecord(M.ev_clear, st);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return e;
  }
  M.ev_pending = true;
  if (M.clear_wanted) {
    M.rot.young_calls = 0;
    M.clears++;
  } else {
    M.rot.rotate();
  }
  M.clear_wanted = M.rotate_wanted = false;
  return hipSuccess;
}

bool memo_pass_begin(mbft_ctx* g, hipStream_t st, uint64_t calls, MemoView* v) {
  VerifiedMemo* M = tabs(g)->memo;
  if (!M || g->memo_guards <= 0) return false;
  std::lock_guard<std::mutex> lk(M->m);
  if (!M->tab || M->rotate_wanted || M->clear_wanted) return false;
  if (M->ev_pending) {  // the last clear ran on another pass's stream
    if (hipEventQuery(M->ev_clear) == hipSuccess) {
      M->ev_pending = false;
    } else {
      (void)hipGetLastError();
      if (hipStreamWaitEvent(st, M->ev_clear, 0) != hipSuccess) {
        (void)hipGetLastError();
        return false;
      }
    }
  }
  M->inflight++;
  const size_t gen_words = (size_t)M->rot.entries * mbft::kMemoEntryWords;
  v->young = M->tab + (size_t)M->rot.young * gen_words;
  v->old = M->tab + (size_t)(M->rot.young ^ 1) * gen_words;
  v->entries = M->rot.entries;
  v->stats = M->d_stats;
  g->memo_open.push_back(MemoOpen{M, st, calls});
  return true;
}

void memo_pass_end(mbft_ctx* g) {
  for (const MemoOpen& o : g->memo_open) {
    // (the callers have synchronized already; after an error they may not have)
    if (hipStreamSynchronize(o.st) != hipSuccess) (void)hipGetLastError();
    std::lock_guard<std::mutex> lk(o.memo->m);
    if (o.memo->rot.add(o.calls)) o.memo->rotate_wanted = true;
    // (a clear that fails here leaves its flag set: the memo stays out of use and the next quiet moment tries again)
    if (--o.memo->inflight == 0 && (o.memo->rotate_wanted || o.memo->clear_wanted))
      (void)memo_clear_quiet(*o.memo, o.st);
  }
  g->memo_open.clear();
}

int memo_clear_engine(mbft_ctx* c, mbft_ctx* e) {
  VerifiedMemo* M = e->memo;
  if (!M) return MBFT_OK;
  if (hipSetDevice(e->device) != hipSuccess) return fail(c, MBFT_ERR_HIP, "hipSetDevice");
  std::lock_guard<std::mutex> lk(M->m);
  if (!M->tab) return MBFT_OK;
  M->clear_wanted = true;
  if (M->inflight == 0) {
    HIPCHK(c, memo_clear_quiet(*M, e->kstream));
    HIPCHK(c, hipStreamSynchronize(e->kstream));
  }
  return MBFT_OK;
}

// An empty table of two generations of `entries`, its counters and its event
// into *M, on engine e's device (current).  On failure what was allocated
// stays in *M for the caller to free.
static int memo_fill(mbft_ctx* c, mbft_ctx* e, uint64_t entries, VerifiedMemo* M) {
  const size_t bytes = 2 * (size_t)entries * mbft::kMemoEntryBytes;
  M->rot.entries = entries;
  if (hipMalloc(&M->tab, bytes) != hipSuccess ||
      hipMalloc(&M->d_stats, mbft_launch::kMemoStats * sizeof(uint64_t)) != hipSuccess) {
    (void)hipGetLastError();
    return fail(c, MBFT_ERR_NOMEM, "verified-call memo: out of device memory");
  }
  // (kstream: never the null stream, see host_internal.h)
  HIPCHK(c, hipEventCreateWithFlags(&M->ev_clear, hipEventDisableTiming));
  HIPCHK(c, hipMemsetAsync(M->tab, 0, bytes, e->kstream));
  HIPCHK(c, hipMemsetAsync(M->d_stats, 0, mbft_launch::kMemoStats * sizeof(uint64_t), e->kstream));
  HIPCHK(c, hipStreamSynchronize(e->kstream));
  return MBFT_OK;
}

int memo_alloc_engine(mbft_ctx* c, mbft_ctx* e, uint64_t entries) {
  if (hipSetDevice(e->device) != hipSuccess) return fail(c, MBFT_ERR_HIP, "hipSetDevice");
  memo_free(e);
  e->memo = new VerifiedMemo;
  const int rc = memo_fill(c, e, entries, e->memo);
  if (rc) memo_free(e);
  return rc;
}

void memo_free(mbft_ctx* e) {
  VerifiedMemo* M = e->memo;
  if (!M) return;
  if (M->tab) (void)hipFree(M->tab);
  if (M->d_stats) (void)hipFree(M->d_stats);
  if (M->ev_clear) (void)hipEventDestroy(M->ev_clear);
  delete M;
  e->memo = nullptr;
}

void count_resident_use(mbft_ctx* c, uint32_t slot, uint8_t status) {
  if (!c->accounting.load(std::memory_order_relaxed)) return;
  if (slot >= c->keydesc.size() || !c->keydesc[slot].valid) return;
  std::lock_guard<std::mutex> g(c->acct_mu);
  if (c->res_uses.size() <= slot) {
    c->res_uses.resize(c->keydesc.size(), 0);
    c->res_rejects.resize(c->keydesc.size(), 0);
  }
  c->res_uses[slot]++;
  if (status != MBFT_ACCEPT) c->res_rejects[slot]++;
}

namespace {

// The streams the library launches engine e's batches on, its lanes' among
// them, have finished (device set): every add of theirs is in the counters.
int sync_engine_streams(mbft_ctx* c, mbft_ctx* e) {
  std::vector<mbft_ctx*> own{e};
  for (mbft_ctx* l : c->lanes)
    if (l->owner == e) own.push_back(l);
  for (mbft_ctx* o : own)
    for (hipStream_t st : {o->stream, o->vstream[0], o->vstream[1]})
      if (st) HIPCHK(c, hipStreamSynchronize(st));
  return MBFT_OK;
}

// Every slot's counts summed over the engines and the resident counter
// (caller holds KeyWriteGuard: no library batch is in flight; the streams the
// library launches on are synchronized here).
int read_usage(mbft_ctx* c, std::vector<uint64_t>& uses, std::vector<uint64_t>& rejects) {
  const size_t ns = c->slots.size();
  uses.assign(ns, 0);
  rejects.assign(ns, 0);
  std::vector<uint64_t> u(ns), r(ns);
  for (mbft_ctx* e : engines_of(c)) {
    if (!e->d_uses || ns == 0) continue;
    if (hipSetDevice(e->device) != hipSuccess) return fail(c, MBFT_ERR_HIP, "hipSetDevice");
    if (const int rc = sync_engine_streams(c, e)) return rc;
    const size_t m = ns < e->acct_slots ? ns : e->acct_slots;
    HIPCHK(c, hipMemcpyAsync(u.data(), e->d_uses, m * sizeof(uint64_t), hipMemcpyDeviceToHost, e->kstream));
    HIPCHK(c, hipMemcpyAsync(r.data(), e->d_rejects, m * sizeof(uint64_t), hipMemcpyDeviceToHost, e->kstream));
    HIPCHK(c, hipStreamSynchronize(e->kstream));
    for (size_t i = 0; i < m; i++) {
      uses[i] += u[i];
      rejects[i] += r[i];
    }
  }
  (void)hipSetDevice(c->device);
  std::lock_guard<std::mutex> g(c->acct_mu);
  for (size_t i = 0; i < c->res_uses.size() && i < ns; i++) {
    uses[i] += c->res_uses[i];
    rejects[i] += c->res_rejects[i];
  }
  return MBFT_OK;
}

// Slot sl's counters back to zero on every engine (a released slot).
int zero_usage(mbft_ctx* c, uint32_t sl) {
  for (mbft_ctx* e : engines_of(c)) {
    if (!e->d_uses || sl >= e->acct_slots) continue;
    if (hipSetDevice(e->device) != hipSuccess) return fail(c, MBFT_ERR_HIP, "hipSetDevice");
    HIPCHK(c, hipMemsetAsync(e->d_uses + sl, 0, sizeof(uint64_t), e->stream));
    HIPCHK(c, hipMemsetAsync(e->d_rejects + sl, 0, sizeof(uint64_t), e->stream));
    HIPCHK(c, hipStreamSynchronize(e->stream));
  }
  (void)hipSetDevice(c->device);
  std::lock_guard<std::mutex> g(c->acct_mu);
  if (sl < c->res_uses.size()) c->res_uses[sl] = c->res_rejects[sl] = 0;
  return MBFT_OK;
}

// Re-class on ONE engine (device set): the new data of every slot in `sl`
// (valid, not yet in cls) is built first, then the descriptors are swapped
// and uploaded, then -- once nothing can read the old data any more -- the old
// storage goes on its class's piece list.  On any failure before the swap
// every key keeps its class.
int reclass_engine(mbft_ctx* c, mbft_ctx* e, const std::vector<uint32_t>& sl, uint32_t cls) {
  const size_t cnt = sl.size();
  if (cnt == 0) return MBFT_OK;
  std::vector<uint32_t> words(16 * cnt);
  for (size_t j = 0; j < cnt; j++) {
    const uint8_t* p = e->slots[sl[j]].xy.data();
    be_to_words(&words[16 * j], p);
    be_to_words(&words[16 * j + 8], p + 32);
  }
  std::vector<uint32_t*> pcs;
  if (const int rc = place_keys(e, cls, words.data(), cnt, cnt, pcs)) return e == c ? rc : fail(c, rc, "peer engine: " + e->err);
  std::vector<mbft::KeyDesc> old(cnt);
  for (size_t j = 0; j < cnt; j++) {
    mbft::KeyDesc& kd = e->keydesc[sl[j]];
    old[j] = kd;
    kd.tab = pcs[j];
    kd.wbits = cls;
    e->kd_dirty.mark(sl[j]);
  }
  if (const int rc = upload_keydesc(e)) {
    // the device may hold either descriptor of a slot, and both point at built
    // data: the host goes back to the old ones (marked, so the next upload
    // restores them on the device) and the new pieces stay out of use until
    // the device has been synchronized -- they go on their list only then
    for (size_t j = 0; j < cnt; j++) {
      e->keydesc[sl[j]] = old[j];
      e->kd_dirty.mark(sl[j]);
    }
    if (hipDeviceSynchronize() == hipSuccess && upload_keydesc(e) == MBFT_OK)
      for (size_t j = 0; j < cnt; j++) e->pieces.release(cls, reinterpret_cast<uintptr_t>(pcs[j]));
    return e == c ? rc : fail(c, rc, "peer engine: " + e->err);
  }
  // the swap is in force on the device: the bookkeeping follows it
  for (size_t j = 0; j < cnt; j++) {
    if (mbft::key_class_queued(old[j].wbits)) e->tfree_keys--;
    e->live_bytes -= mbft::key_class_bytes(old[j].wbits);
  }
  if (mbft::key_class_queued(cls)) e->tfree_keys += cnt;
  e->live_bytes += cnt * mbft::key_class_bytes(cls);
  // (if the synchronize itself fails the device is lost; the old storage is
  // then left off the lists rather than handed out while it may be read)
  if (const int rc = quiesce(c, e)) return rc;
  for (const auto& o : old) e->pieces.release(o.wbits, reinterpret_cast<uintptr_t>(o.tab));
  return MBFT_OK;
}

// The slots of `in` that a re-class into cls has to touch: valid and in
// another class, each once.
std::vector<uint32_t> reclass_list(const mbft_ctx* c, const uint32_t* in, size_t n, uint32_t cls) {
  std::vector<uint32_t> sl;
  for (size_t i = 0; i < n; i++) {
    const uint32_t s = in[i];
    if (s < c->keydesc.size() && c->keydesc[s].valid && c->keydesc[s].wbits != cls) sl.push_back(s);
  }
  std::sort(sl.begin(), sl.end());
  sl.erase(std::unique(sl.begin(), sl.end()), sl.end());
  return sl;
}

int reclass(mbft_ctx* c, const std::vector<uint32_t>& sl, uint32_t cls) {
  if (sl.empty()) return MBFT_OK;
  int rc = MBFT_OK;
  for (mbft_ctx* e : engines_of(c)) {
    std::unique_lock<std::mutex> g(e->mu, std::defer_lock);
    if (e != c) g.lock();
    if (hipSetDevice(e->device) != hipSuccess) return fail(c, MBFT_ERR_HIP, "hipSetDevice");
    rc = reclass_engine(c, e, sl, cls);
    if (rc) break;
  }
  (void)hipSetDevice(c->device);
  c->key_gen++;
  return rc;
}

bool slot_in_use(const mbft_ctx* c, uint32_t sl) {
  return (sl < c->slot_refs.size() && c->slot_refs[sl] != 0) || (sl < c->slot_raw.size() && c->slot_raw[sl] != 0);
}

// The slots of `sl` have no user left: invalid on every engine, their storage
// on the piece lists, their numbers on the free list, their counters zero.
// One descriptor upload and one device synchronize an engine, however many.
int release_slots(mbft_ctx* c, const std::vector<uint32_t>& sl) {
  if (sl.empty()) return MBFT_OK;
  for (mbft_ctx* e : engines_of(c)) {
    std::unique_lock<std::mutex> g(e->mu, std::defer_lock);
    if (e != c) g.lock();
    if (hipSetDevice(e->device) != hipSuccess) return fail(c, MBFT_ERR_HIP, "hipSetDevice");
    std::vector<mbft::KeyDesc> was;
    for (uint32_t s : sl) {
      mbft::KeyDesc& kd = e->keydesc[s];
      was.push_back(kd);
      kd.tab = nullptr;
      kd.valid = 0;
      e->kd_dirty.mark(s);
    }
    if (const int rc = upload_keydesc(e)) return e == c ? rc : fail(c, rc, "peer engine: " + e->err);
    if (const int rc = quiesce(c, e)) return rc;
    // a released number may come to mean another point: what the memo holds under it goes
    if (const int rc = memo_clear_engine(c, e)) return rc;
    for (size_t j = 0; j < sl.size(); j++) {
      if (was[j].valid) {
        if (mbft::key_class_queued(was[j].wbits)) e->tfree_keys--;
        e->live_bytes -= mbft::key_class_bytes(was[j].wbits);
        e->pieces.release(was[j].wbits, reinterpret_cast<uintptr_t>(was[j].tab));
      }
      e->slot_of_xy.erase(e->slots[sl[j]].xy);
      e->slots[sl[j]].valid = false;
      e->free_slots.release(sl[j]);
    }
  }
  (void)hipSetDevice(c->device);
  c->key_gen++;
  for (uint32_t s : sl)
    if (const int rc = zero_usage(c, s)) return rc;
  return MBFT_OK;
}

// ----------------------------------------------------------- the memory budget
// The key store as the ranking kernels read it (key_rank.hip), on the
// context's own device: its descriptors, and as `parts` every array of use
// counts there is -- this engine's own where it stands, the peers' copied
// into rank_parts (directly, through the host if that fails), the resident
// verifier's host-side counts uploaded.  Parts past kRankParts are added into
// the last one.  Every library stream is synchronized first, as read_usage
// does.  Returns with kstream idle.
int rank_store(mbft_ctx* c, const uint32_t* ladder, size_t nladder, mbft_launch::KeyRank& R) {
  using mbft_launch::kRankParts;
  if (hipSetDevice(c->device) != hipSuccess) return fail(c, MBFT_ERR_HIP, "hipSetDevice");
  if (const int rc = upload_keydesc(c)) return rc;
  const size_t ns = c->keydesc.size();
  R = mbft_launch::KeyRank{};
  R.keys = c->d_keys.as<mbft::KeyDesc>();
  R.nslots = (uint32_t)ns;
  R.nladder = (int)nladder;
  for (size_t j = 0; j < nladder; j++) R.ladder[j] = ladder[j];
  if (ns == 0) return MBFT_OK;
  std::vector<uint64_t> res;
  {
    std::lock_guard<std::mutex> g(c->acct_mu);
    res.assign(c->res_uses.begin(), c->res_uses.begin() + std::min(ns, c->res_uses.size()));
  }
  const std::vector<mbft_ctx*> engines = engines_of(c);
  size_t nscratch = res.empty() ? 0 : 1;
  for (mbft_ctx* e : engines)
    if (e->d_uses && (e != c || e->acct_slots < ns)) nscratch++;
  uint64_t* scratch = nullptr;
  if (nscratch) {
    HIPCHK(c, c->rank_parts.ensure(nscratch * ns * sizeof(uint64_t)));
    scratch = c->rank_parts.as<uint64_t>();
    HIPCHK(c, hipMemsetAsync(scratch, 0, nscratch * ns * sizeof(uint64_t), c->kstream));
    HIPCHK(c, hipStreamSynchronize(c->kstream));
  }
  std::vector<const uint64_t*> src;
  std::vector<uint64_t> via;
  size_t used = 0;  // parts of scratch taken
  for (mbft_ctx* e : engines) {
    if (!e->d_uses) continue;
    if (hipSetDevice(e->device) != hipSuccess) return fail(c, MBFT_ERR_HIP, "hipSetDevice");
    if (const int rc = sync_engine_streams(c, e)) return rc;
    if (e == c && e->acct_slots >= ns) {
      src.push_back(e->d_uses);
      continue;
    }
    uint64_t* dst = scratch + used++ * ns;
    const size_t bytes = std::min(ns, e->acct_slots) * sizeof(uint64_t);
    if (hipSetDevice(c->device) != hipSuccess) return fail(c, MBFT_ERR_HIP, "hipSetDevice");
    hipError_t err = e->device == c->device
                         ? hipMemcpyAsync(dst, e->d_uses, bytes, hipMemcpyDeviceToDevice, c->kstream)
                         : hipMemcpyPeerAsync(dst, c->device, e->d_uses, e->device, bytes, c->kstream);
    if (err == hipSuccess) err = hipStreamSynchronize(c->kstream);
    if (err != hipSuccess) {  // no direct path between the two devices: through the host
      (void)hipGetLastError();
      via.resize(bytes / sizeof(uint64_t));
      if (hipSetDevice(e->device) != hipSuccess) return fail(c, MBFT_ERR_HIP, "hipSetDevice");
      HIPCHK(c, hipMemcpyAsync(via.data(), e->d_uses, bytes, hipMemcpyDeviceToHost, e->kstream));
      HIPCHK(c, hipStreamSynchronize(e->kstream));
      if (hipSetDevice(c->device) != hipSuccess) return fail(c, MBFT_ERR_HIP, "hipSetDevice");
      HIPCHK(c, hipMemcpyAsync(dst, via.data(), bytes, hipMemcpyHostToDevice, c->kstream));
      HIPCHK(c, hipStreamSynchronize(c->kstream));
    }
    src.push_back(dst);
  }
  if (hipSetDevice(c->device) != hipSuccess) return fail(c, MBFT_ERR_HIP, "hipSetDevice");
  if (!res.empty()) {
    uint64_t* dst = scratch + used * ns;
    HIPCHK(c, hipMemcpyAsync(dst, res.data(), res.size() * sizeof(uint64_t), hipMemcpyHostToDevice, c->kstream));
    HIPCHK(c, hipStreamSynchronize(c->kstream));
    src.push_back(dst);
  }
  // (src[0] is this engine's own array or scratch, every later one scratch: the sum goes into scratch)
  for (size_t k = kRankParts; k < src.size(); k++)
    HIPCHK(c, mbft_launch::key_add(const_cast<uint64_t*>(src[kRankParts - 1]), src[k], ns, c->kstream));
  HIPCHK(c, hipStreamSynchronize(c->kstream));
  R.nparts = (int)std::min(src.size(), (size_t)kRankParts);
  for (int p = 0; p < R.nparts; p++) R.part[p] = src[(size_t)p];
  return MBFT_OK;
}

}  // namespace

int release_if_unused(mbft_ctx* c, uint32_t sl) {
  if (sl >= c->slots.size() || slot_in_use(c, sl) || c->free_slots.holds(sl)) return MBFT_OK;
  return release_slots(c, {sl});
}

}  // namespace mbft_host

using namespace mbft_host;

extern "C" {

int mbft_set_key_accounting(mbft_ctx* c, int enabled) {
  if (!c || c->owner) return MBFT_ERR_ARG;
  KeyWriteGuard g(c);
  for (mbft_ctx* e : engines_of(c)) {
    if (enabled) {
      if (hipSetDevice(e->device) != hipSuccess) return fail(c, MBFT_ERR_HIP, "hipSetDevice");
      if (const int rc = grow_key_counters(e)) {
        (void)hipSetDevice(c->device);
        return e == c ? rc : fail(c, rc, "peer engine: " + e->err);
      }
    }
    e->accounting.store(enabled != 0);
  }
  (void)hipSetDevice(c->device);
  return MBFT_OK;
}

int mbft_key_usage(mbft_ctx* c, const uint32_t* slots, size_t n, uint64_t* uses_out, uint64_t* rejects_out) {
  if (!c || c->owner) return MBFT_ERR_ARG;
  KeyWriteGuard g(c);
  std::vector<uint64_t> u, r;
  if (const int rc = read_usage(c, u, r)) return rc;
  for (size_t i = 0; i < n; i++) {
    const size_t s = slots ? slots[i] : i;
    if (uses_out) uses_out[i] = s < u.size() ? u[s] : 0;
    if (rejects_out) rejects_out[i] = s < r.size() ? r[s] : 0;
  }
  return MBFT_OK;
}

int mbft_reset_key_usage(mbft_ctx* c) {
  if (!c || c->owner) return MBFT_ERR_ARG;
  KeyWriteGuard g(c);
  for (mbft_ctx* e : engines_of(c)) {
    if (!e->d_uses) continue;
    if (hipSetDevice(e->device) != hipSuccess) return fail(c, MBFT_ERR_HIP, "hipSetDevice");
    if (const int rc = quiesce(c, e)) return rc;  // adds still in flight belong to the old count
    HIPCHK(c, hipMemset(e->d_uses, 0, e->acct_slots * sizeof(uint64_t)));
    HIPCHK(c, hipMemset(e->d_rejects, 0, e->acct_slots * sizeof(uint64_t)));
  }
  (void)hipSetDevice(c->device);
  std::lock_guard<std::mutex> am(c->acct_mu);
  std::fill(c->res_uses.begin(), c->res_uses.end(), 0);
  std::fill(c->res_rejects.begin(), c->res_rejects.end(), 0);
  return MBFT_OK;
}

int mbft_get_key_class(const mbft_ctx* c, uint32_t role, uint32_t id, uint32_t* cls, uint64_t* table_bytes) {
  if (!c) return MBFT_ERR_ARG;
  const int sl = mbft_key_slot(c, role, id);
  if (sl < 0) return sl;
  if ((size_t)sl >= c->keydesc.size()) return MBFT_ERR_STATE;
  const mbft::KeyDesc& kd = c->keydesc[(size_t)sl];
  if (cls) *cls = kd.wbits;
  if (table_bytes) *table_bytes = kd.valid ? mbft::key_class_bytes(kd.wbits) : 0;
  return MBFT_OK;
}

int mbft_set_slot_classes(mbft_ctx* c, const uint32_t* slots, size_t n, uint32_t cls) {
  if (!c || c->owner || (n && !slots) || !mbft::key_class_known(cls)) return MBFT_ERR_ARG;
  KeyWriteGuard g(c);
  for (size_t i = 0; i < n; i++)
    if (slots[i] >= c->keydesc.size()) return fail(c, MBFT_ERR_ARG, "mbft_set_slot_classes: no such slot");
  return reclass(c, reclass_list(c, slots, n, cls), cls);
}

int mbft_set_key_class(mbft_ctx* c, uint32_t role, uint32_t id, uint32_t cls) {
  if (!c || c->owner || !mbft::key_class_known(cls)) return MBFT_ERR_ARG;
  KeyWriteGuard g(c);
  const int sl = mbft_key_slot(c, role, id);
  if (sl < 0) return sl;
  const uint32_t s = (uint32_t)sl;
  if (s >= c->keydesc.size() || !c->keydesc[s].valid) return fail(c, MBFT_ERR_ARG, "mbft_set_key_class: invalid slot");
  return reclass(c, reclass_list(c, &s, 1, cls), cls);
}

int mbft_promote_hot_keys(mbft_ctx* c, uint32_t cls, size_t max_keys, uint64_t min_uses, size_t* promoted) {
  if (promoted) *promoted = 0;
  if (!c || c->owner || !mbft::key_class_known(cls)) return MBFT_ERR_ARG;
  KeyWriteGuard g(c);
  std::vector<uint64_t> u, r;
  if (const int rc = read_usage(c, u, r)) return rc;
  const size_t ns = c->keydesc.size();
  std::vector<uint32_t> co(ns);
  std::vector<uint8_t> valid(ns);
  for (size_t i = 0; i < ns; i++) {
    co[i] = c->keydesc[i].wbits;
    valid[i] = c->keydesc[i].valid ? 1 : 0;
  }
  const std::vector<uint32_t> pick = mbft::promotion_choice(u.data(), co.data(), valid.data(), ns, cls, max_keys, min_uses);
  const int rc = reclass(c, reclass_list(c, pick.data(), pick.size(), cls), cls);
  if (rc == MBFT_OK && promoted) *promoted = pick.size();
  return rc;
}

int mbft_remove_public_key(mbft_ctx* c, uint32_t role, uint32_t id) {
  if (!c || c->owner) return MBFT_ERR_ARG;
  KeyWriteGuard g(c);
  auto rs = c->roles.find(role);
  if (rs == c->roles.end()) return MBFT_ERR_KEY;
  auto it = rs->second.find(id);
  if (it == rs->second.end()) return MBFT_ERR_KEY;
  const uint32_t sl = it->second.slot;
  rs->second.erase(it);
  c->key_gen++;
  if (sl < c->slot_refs.size() && c->slot_refs[sl]) c->slot_refs[sl]--;
  return release_if_unused(c, sl);
}

int mbft_release_slots(mbft_ctx* c, const uint32_t* slots, size_t n) {
  if (!c || c->owner || (n && !slots)) return MBFT_ERR_ARG;
  KeyWriteGuard g(c);
  for (size_t i = 0; i < n; i++)
    if (slots[i] >= c->slots.size()) return fail(c, MBFT_ERR_ARG, "mbft_release_slots: no such slot");
  std::vector<uint32_t> gone;
  for (size_t i = 0; i < n; i++) {
    const uint32_t sl = slots[i];
    if (sl < c->slot_raw.size()) c->slot_raw[sl] = 0;
    if (!slot_in_use(c, sl) && !c->free_slots.holds(sl)) gone.push_back(sl);
  }
  std::sort(gone.begin(), gone.end());
  gone.erase(std::unique(gone.begin(), gone.end()), gone.end());
  return release_slots(c, gone);
}

int mbft_key_memory(const mbft_ctx* c, uint64_t out[3]) {
  if (!c || !out) return MBFT_ERR_ARG;
  out[0] = c->live_bytes;
  out[1] = c->pieces.bytes();
  uint64_t blocks = 0;
  for (size_t b : c->tab_sizes) blocks += b;
  out[2] = blocks;
  return MBFT_OK;
}

int mbft_age_key_usage(mbft_ctx* c, unsigned shift) {
  if (!c || c->owner || shift >= 64) return MBFT_ERR_ARG;
  if (shift == 0) return MBFT_OK;
  KeyWriteGuard g(c);
  for (mbft_ctx* e : engines_of(c)) {
    if (!e->d_uses) continue;
    if (hipSetDevice(e->device) != hipSuccess) return fail(c, MBFT_ERR_HIP, "hipSetDevice");
    if (const int rc = sync_engine_streams(c, e)) return rc;  // adds still in flight belong to the old count
    HIPCHK(c, mbft_launch::key_age(e->d_uses, e->d_rejects, e->acct_slots, shift, e->kstream));
    HIPCHK(c, hipStreamSynchronize(e->kstream));
  }
  (void)hipSetDevice(c->device);
  std::lock_guard<std::mutex> am(c->acct_mu);
  for (uint64_t& v : c->res_uses) v >>= shift;
  for (uint64_t& v : c->res_rejects) v >>= shift;
  return MBFT_OK;
}

int mbft_set_key_budget(mbft_ctx* c, uint64_t bytes) {
  if (!c || c->owner) return MBFT_ERR_ARG;
  KeyWriteGuard g(c);
  c->key_budget = bytes;
  return MBFT_OK;
}

int mbft_get_key_budget(const mbft_ctx* c, uint64_t* bytes) {
  if (!c || !bytes) return MBFT_ERR_ARG;
  *bytes = c->key_budget;
  return MBFT_OK;
}

int mbft_set_verified_memo(mbft_ctx* c, uint64_t bytes) {
  if (!c || c->owner) return MBFT_ERR_ARG;
  const mbft::MemoGeometry geo = mbft::memo_geometry(bytes);
  if (bytes != 0 && geo.entries == 0)
    return fail(c, MBFT_ERR_ARG, "mbft_set_verified_memo: below the minimum of 2 x 1,024 entries");
  KeyWriteGuard g(c);  // no pass is in flight
  const std::vector<mbft_ctx*> eng = engines_of(c);
  std::vector<VerifiedMemo*> fresh;
  int rc = MBFT_OK;
  if (bytes != 0) {
    for (mbft_ctx* e : eng) {
      if (hipSetDevice(e->device) != hipSuccess) {
        rc = fail(c, MBFT_ERR_HIP, "hipSetDevice");
        break;
      }
      VerifiedMemo* M = new VerifiedMemo;
      fresh.push_back(M);
      if ((rc = memo_fill(c, e, geo.entries, M)) != MBFT_OK) break;
    }
  }
  // everything that can fail comes before the first engine changes: the streams
  // that may still run a pass's kernels on an old memo have finished
  for (size_t j = 0; j < eng.size() && !rc; j++) {
    if (!eng[j]->memo) continue;
    if (hipSetDevice(eng[j]->device) != hipSuccess)
      rc = fail(c, MBFT_ERR_HIP, "hipSetDevice");
    else
      rc = sync_engine_streams(c, eng[j]);
  }
  if (rc) {  // the previous state stays
    for (size_t j = 0; j < fresh.size(); j++) {
      if (hipSetDevice(eng[j]->device) != hipSuccess) (void)hipGetLastError();
      if (fresh[j]->tab) (void)hipFree(fresh[j]->tab);
      if (fresh[j]->d_stats) (void)hipFree(fresh[j]->d_stats);
      if (fresh[j]->ev_clear) (void)hipEventDestroy(fresh[j]->ev_clear);
      delete fresh[j];
    }
    (void)hipSetDevice(c->device);
    return rc;
  }
  for (size_t j = 0; j < eng.size(); j++) {
    if (hipSetDevice(eng[j]->device) != hipSuccess) (void)hipGetLastError();
    memo_free(eng[j]);
    if (bytes != 0) eng[j]->memo = fresh[j];
  }
  (void)hipSetDevice(c->device);
  return MBFT_OK;
}

int mbft_get_verified_memo(mbft_ctx* c, uint64_t* bytes) {
  if (!c || c->owner || !bytes) return MBFT_ERR_ARG;
  std::shared_lock<std::shared_mutex> t(c->tab_mu);
  *bytes = c->memo ? 2u * c->memo->rot.entries * mbft::kMemoEntryBytes : 0u;
  return MBFT_OK;
}

int mbft_verified_memo_stats(mbft_ctx* c, uint64_t out[6]) {
  if (!c || c->owner || !out) return MBFT_ERR_ARG;
  std::shared_lock<std::shared_mutex> t(c->tab_mu);
  for (int k = 0; k < 6; k++) out[k] = 0;
  for (mbft_ctx* e : engines_of(c)) {
    VerifiedMemo* M = e->memo;
    if (!M) continue;
    if (hipSetDevice(e->device) != hipSuccess) return MBFT_ERR_HIP;
    uint64_t v[mbft_launch::kMemoStats];
    if (hipMemcpyAsync(v, M->d_stats, sizeof(v), hipMemcpyDeviceToHost, e->kstream) != hipSuccess ||
        hipStreamSynchronize(e->kstream) != hipSuccess) {
      (void)hipGetLastError();
      (void)hipSetDevice(c->device);
      return MBFT_ERR_HIP;
    }
    for (int k = 0; k < mbft_launch::kMemoStats; k++) out[k] += v[k];
    std::lock_guard<std::mutex> lk(M->m);
    out[4] += M->rot.rotations;
    out[5] += M->clears;
  }
  (void)hipSetDevice(c->device);
  return MBFT_OK;
}

int mbft_clear_verified_memo(mbft_ctx* c) {
  if (!c || c->owner) return MBFT_ERR_ARG;
  std::shared_lock<std::shared_mutex> t(c->tab_mu);  // (the memo is not replaced meanwhile; passes go on)
  for (mbft_ctx* e : engines_of(c))
    if (const int rc = memo_clear_engine(c, e)) return rc;
  (void)hipSetDevice(c->device);
  return MBFT_OK;
}

uint32_t mbft_key_class_cost(uint32_t cls) { return mbft::key_class_cost(cls); }

int mbft_rebalance_keys(mbft_ctx* c, const uint32_t* ladder, size_t nladder, uint64_t min_uses,
                        mbft_rebalance_result* out) {
  using namespace mbft_launch;
  if (out) *out = mbft_rebalance_result{};
  if (!c || c->owner || !out || !mbft::rebalance_ladder_ok(ladder, nladder)) return MBFT_ERR_ARG;
  KeyWriteGuard g(c);
  // (counts that are all zero would demote every key)
  if (!c->accounting.load()) return fail(c, MBFT_ERR_STATE, "mbft_rebalance_keys: key accounting is off");
  if (c->key_budget == 0) return fail(c, MBFT_ERR_STATE, "mbft_rebalance_keys: no key budget is set");
  const int L = (int)nladder;
  KeyRank R;
  if (const int rc = rank_store(c, ladder, nladder, R)) return rc;
  out->live_before = out->live_after = c->live_bytes;
  // the histogram: a few kilobytes, whatever the slots
  HIPCHK(c, c->rank_out.ensure(sizeof(uint32_t) * (kRankHistWords + kRankLadder) + kRankBins));
  uint32_t* d_hist = c->rank_out.as<uint32_t>();
  uint32_t* d_count = d_hist + kRankHistWords;
  uint8_t* d_rob = reinterpret_cast<uint8_t*>(d_count + kRankLadder);
  std::vector<uint32_t> hist(kRankHistWords);
  HIPCHK(c, key_hist(R, d_hist, c->kstream));
  HIPCHK(c, hipMemcpyAsync(hist.data(), d_hist, sizeof(uint32_t) * kRankHistWords, hipMemcpyDeviceToHost, c->kstream));
  HIPCHK(c, hipStreamSynchronize(c->kstream));
  uint64_t of_bin[kRankBins] = {}, ladder_bytes = 0;
  for (int j = 0; j < L; j++)
    for (int b = 0; b < kRankBins; b++) {
      const uint32_t k = hist[(size_t)j * kRankBins + b];
      of_bin[b] += k;
      out->keys_per_rung[j] += k;
      ladder_bytes += k * mbft::key_class_bytes(ladder[j]);
    }
  // valid keys outside the ladder are pinned: they keep their class and their bytes count
  out->pinned_bytes = c->live_bytes - ladder_bytes;
  const uint64_t avail = c->key_budget > out->pinned_bytes ? c->key_budget - out->pinned_bytes : 0;
  const mbft::RebalancePlan plan = mbft::rebalance_plan(of_bin, ladder, nladder, avail, min_uses);
  if (plan.excess) out->over_budget = out->pinned_bytes + plan.bytes - c->key_budget;
  // every list's length is known from the histogram: the slots of another rung in the bins that go to t
  KeyPickLists lists{};
  size_t moving = 0;
  for (int b = 0; b < kRankBins; b++)
    for (int j = 0; j < L; j++)
      if (j != plan.rung_of_bin[b]) lists.cap[plan.rung_of_bin[b]] += hist[(size_t)j * kRankBins + b];
  for (int t = 0; t < L; t++) moving += lists.cap[t];
  if (moving == 0) return MBFT_OK;
  HIPCHK(c, c->rank_lists.ensure(moving * sizeof(uint32_t)));
  for (size_t t = 0, off = 0; t < nladder; off += lists.cap[t++]) lists.list[t] = c->rank_lists.as<uint32_t>() + off;
  HIPCHK(c, hipMemcpyAsync(d_rob, plan.rung_of_bin, kRankBins, hipMemcpyHostToDevice, c->kstream));
  HIPCHK(c, key_pick_plan(R, d_rob, lists, d_count, c->kstream));
  uint32_t count[kRankLadder];
  std::vector<uint32_t> moved(moving);
  HIPCHK(c, hipMemcpyAsync(count, d_count, sizeof(count), hipMemcpyDeviceToHost, c->kstream));
  HIPCHK(c, hipMemcpyAsync(moved.data(), c->rank_lists.p, moving * sizeof(uint32_t), hipMemcpyDeviceToHost, c->kstream));
  HIPCHK(c, hipStreamSynchronize(c->kstream));
  for (int t = 0; t < L; t++)
    if (count[t] != lists.cap[t]) return fail(c, MBFT_ERR_STATE, "mbft_rebalance_keys: the lists disagree with the histogram");
  // per target rung the keys that come down to it and those that go up to it, each ascending
  std::vector<uint32_t> down[kRankLadder], up[kRankLadder];
  for (size_t t = 0, off = 0; t < nladder; off += lists.cap[t++])
    for (size_t k = off; k < off + lists.cap[t]; k++) {
      const uint32_t s = moved[k];
      if (s >= c->keydesc.size() || !c->keydesc[s].valid ||
          std::find(ladder, ladder + nladder, c->keydesc[s].wbits) == ladder + nladder)
        return fail(c, MBFT_ERR_STATE, "mbft_rebalance_keys: a listed slot is not a ladder key");
      (mbft::key_class_bytes(c->keydesc[s].wbits) > mbft::key_class_bytes(ladder[t]) ? down[t] : up[t]).push_back(s);
    }
  // demotions first, rung 0 upwards, then promotions from the top rung downwards: the promotions take the
  // pieces the demotions released.  A failure stops the walk; every bulk step is all or nothing.
  int rc = MBFT_OK;
  auto step = [&](std::vector<uint32_t>& sl, int t, uint32_t* tally) {
    if (rc != MBFT_OK || sl.empty()) return;
    std::sort(sl.begin(), sl.end());
    std::vector<int> from(sl.size());
    for (size_t k = 0; k < sl.size(); k++)
      from[k] = (int)(std::find(ladder, ladder + nladder, c->keydesc[sl[k]].wbits) - ladder);
    rc = reclass(c, sl, ladder[t]);
    if (rc != MBFT_OK) return;
    for (int j : from) out->keys_per_rung[j]--;
    out->keys_per_rung[t] += (uint32_t)sl.size();
    *tally += (uint32_t)sl.size();
  };
  for (int t = 0; t < L; t++) step(down[t], t, &out->demoted);
  for (int t = L - 1; t >= 0; t--) step(up[t], t, &out->promoted);
  out->live_after = c->live_bytes;
  return rc;
}

int mbft_cold_keys(mbft_ctx* c, uint64_t max_uses, uint32_t* slots_out, size_t cap, size_t* count) {
  using namespace mbft_launch;
  if (count) *count = 0;
  if (!c || c->owner || !count || (cap && !slots_out)) return MBFT_ERR_ARG;
  KeyWriteGuard g(c);
  KeyRank R;
  if (const int rc = rank_store(c, nullptr, 0, R)) return rc;
  if (R.nslots == 0) return MBFT_OK;
  HIPCHK(c, c->rank_out.ensure(sizeof(uint32_t) * (kRankHistWords + kRankLadder) + kRankBins));
  uint32_t* d_count = c->rank_out.as<uint32_t>();
  // room for `cap` first; if more are cold, once more with room for all, so that the cap LOWEST are returned
  uint32_t room = (uint32_t)std::min<size_t>(cap, R.nslots), total = 0;
  std::vector<uint32_t> cold;
  for (int pass = 0; pass < 2; pass++) {
    HIPCHK(c, c->rank_lists.ensure((room ? room : 1) * sizeof(uint32_t)));
    HIPCHK(c, key_pick_cold(R, max_uses, c->rank_lists.as<uint32_t>(), room, d_count, c->kstream));
    HIPCHK(c, hipMemcpyAsync(&total, d_count, sizeof(total), hipMemcpyDeviceToHost, c->kstream));
    HIPCHK(c, hipStreamSynchronize(c->kstream));
    if (total <= room || cap == 0) break;
    room = total;
  }
  *count = total;
  cold.resize(std::min(room, total));
  if (!cold.empty()) {
    HIPCHK(c, hipMemcpyAsync(cold.data(), c->rank_lists.p, cold.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, c->kstream));
    HIPCHK(c, hipStreamSynchronize(c->kstream));
  }
  std::sort(cold.begin(), cold.end());
  for (size_t k = 0; k < cold.size() && k < cap; k++) slots_out[k] = cold[k];
  return MBFT_OK;
}

}  // extern "C"
