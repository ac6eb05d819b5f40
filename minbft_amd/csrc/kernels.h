// Host-side launch wrappers for the kernels of every .hip unit: the one header
// the host units include.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "verify_plan.h"

namespace mbft {
// Per key slot, read by k_verify (16 B): the key's comb table, its window and
// whether the key passed validation.  A table-free key (window 0): tab is the
// point as one comb entry, wbits 0.  A compact key (t teeth, teeth_dev.h): tab
// is its table of 2^t entries, wbits kTeethFlag | t -- a class code, NOT a
// window: whatever takes wbits as a comb window first rules it out with
// key_class_queued.
struct KeyDesc {
  const uint32_t* tab;
  uint32_t wbits;
  uint32_t valid;
};
constexpr uint32_t kTeethFlag = 0x100u;
// A signed compact key (t = 2 .. 9 teeth, teeth_dev.h): tab is its table of
// 2^(t-1) entries, wbits kSignedTeethFlag | t -- a class code like the
// compact one's, queued like it (>= kTeethFlag).
constexpr uint32_t kSignedTeethFlag = 0x200u;
// The key classes that take no part in the comb: window 0 and the compact
// class.  k_verify queues their items for k_verify_ladder, the small-batch
// kernels serve them in place (verify_ladder_inline), the resident verifier
// hands them to the ordinary path.
__host__ __device__ inline bool key_class_queued(uint32_t wbits) {
  return wbits == 0u || wbits >= kTeethFlag;
}
// Key slots >= kHostSlot carry a status the host decided for the item
// (batch pipeline): k_verify writes the slot's low byte as the status.
constexpr uint32_t kHostSlot = 0xFFFFFF00u;
}  // namespace mbft

namespace mbft {
// One ECDSA input e built on the GPU from a message's raw fields and the
// SHA-256 of its operation (mbft_validate_messages / _replies; k_authen_e).
enum AuthenKind : uint32_t {
  kAuthenRequest = 0,  // e = ("REQUEST" || seq || H(op) || SHA256(""))[0:32]
  kAuthenReply = 1,    // e = ("REPLY" || client || seq || H(result) || ...)[0:32]
  kAuthenPrepare = 2,  // e = SHA256(SHA256("PREPARE" || view || client || seq || H(op))
                       //            || epoch_le || counter_le)
  kAuthenCommit = 3    // same over "COMMIT" || primary || view || client || seq || H(op) || prep_ctr
};
struct AuthenDesc {
  uint32_t kind, msg;        // kind, index of the message's H(op)
  uint32_t item, client;     // destination item of e; client id
  uint32_t primary, pad;
  uint64_t view, seq, prep_ctr, epoch, counter;
};
}  // namespace mbft

namespace mbft {
// (role, id) -> key slot on the device, for k_prepare: open addressing over
// keys[] = (role << 32) | id (empty: ~0), cap = mask + 1 a power of two at
// load <= 1/2, linear probing.  role_ok bit r: role r has a verification
// scheme in this context (Replica / Client registered; USIG registered and
// enabled), exactly the host's keymanager.go:100 / authenticator.go:126-129
// dispatch.
struct KeyMap {
  const uint64_t* keys;
  const uint32_t* slots;
  uint32_t mask;
  uint32_t role_ok;
};
__host__ __device__ inline uint32_t keymap_hash(uint64_t k) {
  return (uint32_t)((k * 0x9E3779B97F4A7C15ull) >> 32);
}
// Raw VerifyMessageAuthenTag calls i in [0, n) of one chunk, decoded on the
// GPU (mbft_verify_batch_flat over library-owned page-locked buffers): call
// i = (roles[i], ids[i], msgs + moff[i] - mbase .. moff[i + 1] - mbase, tags
// likewise).  Outputs the verifier's items: e, r, s (32 B big-endian each)
// and the key slot, or kHostSlot | status where the call is decided before
// the signature check (kHostSlot | MBFT_BAD_KEY where the host's USIG epoch
// step decides it).
struct PrepArgs {
  const uint32_t* roles;    // wide form (or null: roles8)
  const uint32_t* ids;
  const uint64_t* moff;     // wide form (or null: moff32 / toff32)
  const uint64_t* toff;
  const uint8_t* roles8;    // compact form (mbft_verify_batch_flat32)
  const uint32_t* moff32;
  const uint32_t* toff32;
  const uint8_t* msgs;
  const uint8_t* tags;
  uint64_t mbase, tbase;    // absolute offset of msgs[0] / tags[0]
  uint64_t mlo, mhi, tlo, thi;  // this chunk's byte ranges (absolute): a call outside sets *bad
  uint32_t* bad;
  long n;
  KeyMap map;
  const KeyDesc* keys;
  uint32_t nslots;
  uint8_t* e;
  uint8_t* r;
  uint8_t* s;
  uint32_t* slot;
};
}  // namespace mbft

namespace mbft {
// The resident single-call verifier (k_verify_server, resident.cpp): a kernel
// that stays on the GPU while single calls keep arriving, two 256-thread
// workgroups per mailbox slot in host-mapped memory.  The host fills a slot's
// fields, then its seq (24 bits, never 0); the workgroups see the new seq,
// run the item's comb sums, and write (seq << 8) | status to the slot's done
// words.  No launch and no stream synchronize per call.
constexpr int kSrvMaxSlots = 64;
constexpr int kSrvMaxParts = 16;  // partial sums per item (two workgroups, 8 each)
struct alignas(256) SrvSlot {
  uint32_t seq;           // written last by the host
  uint32_t key0;          // 0: the item's index into kd
  uint32_t wg;            // generator window
  uint32_t ugiven;        // 1: u[] holds u1, u2 (computed by the host)
  const uint32_t* tabG;   // generator comb table (per item: it may be rebuilt)
  uint32_t gjoin;         // 1: the joins and the x test on the GPU, a final status (no partials)
  uint32_t pad1;
  KeyDesc kd;             // the signer's table (offset 32)
  uint8_t e[32], r[32], s[32];  // offsets 48, 80, 112 (16-B aligned)
  uint32_t winv[12];      // s^-1 R mod N, 9 limbs (planes of one item)
  uint32_t u[16];         // u1 = e s^-1, u2 = r s^-1 mod N, 8 LE words each (ugiven)
};
static_assert(sizeof(SrvSlot) == 256 && __builtin_offsetof(SrvSlot, kd) == 32 &&
                  __builtin_offsetof(SrvSlot, e) == 48 && __builtin_offsetof(SrvSlot, winv) == 144 &&
                  __builtin_offsetof(SrvSlot, u) == 192,
              "mailbox slot layout");
// A post's tag from its seq: 1..255, the next post's tag always the
// successor t % 255 + 1 of this one's (seq steps by one per post, skipping
// 0); the servers open a job only for the successor of its claim.
inline uint32_t srv_tag(uint32_t seq) { return seq % 255u + 1u; }
struct SrvCtl {
  // the doorbell line: slot b's post tag in byte b (srv_tag of its seq; 0:
  // never posted), written by the host after the slot and its seq
  uint32_t tag32[kSrvMaxSlots / 4];
  uint32_t exited_gen;    // kernel: the generation that decided to exit
  uint32_t stop_gen;      // host: the generation told to stop (set_resident(0), destroy)
  uint32_t pad1[14];
  // (seq << 8) | status, one cache line per slot: word 0, and word 8 for the
  // second workgroup of the two-workgroup form
  uint32_t done[kSrvMaxSlots][16];
  // status kSrvPartials: the item's partial comb sums, one per wave (G's
  // window ranges, then Q's), 40 words each -- X, Y, ZZ, ZZZ (9 device limbs
  // each, Montgomery form), a flags word (1: infinity) -- for the host to
  // join and x-check (join_host.cpp); 4 sums, or 16 in the two-workgroup form
  // (unused ones flagged infinity)
  uint32_t part[kSrvMaxSlots][kSrvMaxParts * 40];
};
constexpr uint8_t kSrvPartials = 0xFE;
struct ServerArgs {
  SrvCtl* ctl;        // device views of the host-mapped control block
  SrvSlot* slots;     // ... and mailbox
  uint8_t* st;        // device scratch: each slot's status byte
  uint32_t* dexit;    // device: [0] generation told to exit, [2..3] last activity (u64)
  uint32_t* claim;    // device: [half * kSrvMaxSlots + b] the tag of slot b's last claimed job
  uint32_t gen;       // this launch's generation (never 0)
  uint32_t nslots;    // mailbox slots (1..kSrvMaxSlots)
  uint64_t idle_ticks;   // exit after this long without a post (100 MHz ticks)
  uint64_t life_ticks;   // ... or this long after the start
  uint32_t poll_sleep;   // s_sleep(8) steps between two empty doorbell polls (>= 1)
  uint32_t pad;
};
}  // namespace mbft

namespace mbft_launch {

using mbft::AuthenDesc;
using mbft::KeyDesc;
using mbft::PrepArgs;

hipError_t prepare_calls(const PrepArgs& a, hipStream_t st);

// Comb windows: W bits per SIGNED digit, S = ceil(256/W) windows, 2^(W-1)
// affine entries per window (|d|; the last window holds the 2^(256-(S-1)W)
// its digits reach), 64 B per entry.  W = 8 -> 32 mixed additions per
// scalar, 0.25 MiB; 16 -> 16 additions, 34 MiB; 20 -> 13, 388 MiB;
// 22 -> 12, 1.4 GiB; 24 -> 11, 5.0 GiB; 26 -> 10, 18.3 GiB; 29 -> 9, 129 GiB.
constexpr int kMinWindow = 4, kMaxWindow = 29;
// Key window 0 (MBFT_WINDOW_NONE): no table.  The key's KeyDesc.tab points at
// the point itself, ONE entry, and wbits is 0 (ladder_dev.h).  Keys only:
// the generator always has a comb.
constexpr int kWindowNone = 0;
size_t table_entries(int wbits);
size_t table_words(int wbits);
int table_steps(int wbits);

hipError_t sha256_var(const uint8_t* data, const uint64_t* off, long n, uint8_t* out,
                      hipStream_t st);
hipError_t usig_e(const uint8_t* data, const uint64_t* off, const uint64_t* epoch,
                  const uint64_t* counter, const uint32_t* idx, long n, uint8_t* e,
                  hipStream_t st);
hipError_t request_e(const uint64_t* seq, const uint8_t* ops, uint32_t op_len, long n, uint8_t* e,
                     hipStream_t st);
hipError_t authen_e(const uint8_t* H, const AuthenDesc* d, long n, uint8_t* e, hipStream_t st);
hipError_t check_points(const uint32_t* xy, int n, uint32_t* ok, hipStream_t st);
// n validated points -> n comb entries (16 words each): a table-free key's
// whole device state (key window 0)
hipError_t point_entries(const uint32_t* xy, int n, uint32_t* out, hipStream_t st);
hipError_t build_tables(const uint32_t* xy, int npts, int wbits, uint32_t* bpts, uint32_t* tab,
                        hipStream_t st);
// The compact key class (teeth_dev.h): `teeth` in 2 .. 8, a table of 2^teeth
// entries of 16 words per key (entry 0 never read) -- 256 B at 2 teeth, 1 KiB
// at 4, 16 KiB at 8 -- verified by a comb WITH doublings, ceil(256 / teeth)
// columns.  xy: npts validated plain affine points; tab: npts tables, one
// after another, 64-byte aligned.  Returns when the tables are built.
constexpr int kTeethMin = 2, kTeethMax = 8;
size_t teeth_table_words(int teeth);
hipError_t build_teeth_tables(const uint32_t* xy, int npts, int teeth, uint32_t* tab, hipStream_t st);
// The signed compact key class (teeth_dev.h): `teeth` in 2 .. 9, a table of
// 2^(teeth - 1) entries of 16 words per key (every entry read) -- 128 B at 2
// teeth, 1 KiB at 5, 16 KiB at 9.  Arguments as build_teeth_tables.
constexpr int kSteethMin = 2, kSteethMax = 9;
size_t steeth_table_words(int teeth);
hipError_t build_steeth_tables(const uint32_t* xy, int npts, int teeth, uint32_t* tab, hipStream_t st);
hipError_t generator_xy(uint32_t* xy16, hipStream_t st);
size_t ninv_workspace_words(long n);
// One launch, one root inversion per 2,048 items (k_ninv_block, per
// workgroup): for a batch issued while the GPU is idle (latency), not for
// the steady-state pipeline (VALU work).
// zero_word (optional): zeroed by the kernel (the exact-path queue counter
// of the verify that follows on the same stream).
hipError_t batch_inverse_s_local(const uint8_t* s, long n, uint32_t* winv, uint32_t* zero_word,
                                 hipStream_t st);
// The pipelined form (earlier batches in flight): per-wave chains of 16.
hipError_t batch_inverse_s_pipelined(const uint8_t* s, long n, uint32_t* winv, uint32_t* zero_word,
                                     hipStream_t st);
// The level chain for the pipeline (k_ninv_up / k_ninv_top / k_ninv_down);
// zero_word as above (zeroed by the last kernel of the chain).
hipError_t batch_inverse_s(const uint8_t* s, long n, uint32_t* ws, uint32_t* winv,
                           uint32_t* zero_word, hipStream_t st);
hipError_t sign(const uint8_t* priv, const uint32_t* key_idx, const uint8_t* e, const uint8_t* k_in,
                long n, const uint32_t* tabG, int wg, uint8_t* r_out, uint8_t* s_out,
                hipStream_t st);
// One batch for verify(): n items in device memory and the buffers they use.
struct VerifyBatch {
  const uint8_t *e, *r, *s;  // n x 32 B big-endian each
  const uint32_t* slot;     // n key slots
  long n;
  uint8_t* status;
  uint32_t* slowq;          // verify_slowq_words(n, plan) words (verify_plan.h)
  const uint32_t* winv;     // the s^-1 R planes the plan's source names: 9 planes of n, the host's
                            // followed by u1, u2 (16 words an item, batch.cpp host_winv_u); or null
  uint32_t* planes_ws;      // 9 n words for the forms that run k_ninv_local<1> first, or null
  const uint32_t* ndev;     // optional: the item count on the device, <= n
  bool host_status;         // slots >= kHostSlot carry the host's status
};
// The tables a batch is verified under.
struct VerifyTables {
  const uint32_t* tabG;     // generator comb table, window wg
  int wg;
  const KeyDesc* keys;
  uint32_t nslots;
  bool table_free;          // some key is of a class the comb does not serve (key_class_queued)
  uint64_t* uses = nullptr;     // per-slot counters of the plan's use-count stage (nslots entries each;
  uint64_t* rejects = nullptr;  // read only when plan.account is set)
};
// The use-count stage on its own (key_account.hip, k_key_account): per key slot
// the batch's items under it (slot < nslots and KeyDesc.valid) and those of
// them whose status is not MBFT_ACCEPT, ADDED into uses[] / rejects[].  Items
// whose slot word is >= nslots (host-decided words, >= kHostSlot, among them)
// or names an invalid slot are not counted.  ndev (optional): the item count on
// the device, nothing past min(n, *ndev) is read.  verify() launches it last
// where the plan says so.
struct KeyAccount {
  const uint32_t* slot;
  const uint8_t* status;
  long n;
  const uint32_t* ndev;
  const KeyDesc* keys;
  uint32_t nslots;
  uint64_t* uses;
  uint64_t* rejects;
};
hipError_t key_account(const KeyAccount& a, hipStream_t st);
// The verified-call memo's two stages (memo.hip, memo_plan.h; DESIGN.md
// §4.12) around the verify of a pass.  The table: two generations of `entries`
// (a power of two) 128-byte entries each, `young` and `old`.  stats: four
// 64-bit counters on the device -- lookups, hits, inserts, dropped -- added to
// with one relaxed agent-scope atomic a wave.  e, r, s and their compacted
// copies are 16-byte aligned.
constexpr int kMemoStatLookups = 0, kMemoStatHits = 1, kMemoStatInserts = 2, kMemoStatDropped = 3, kMemoStats = 4;
// k_memo_probe, one item per lane: an item under a real valid key (slot <
// nslots and KeyDesc.valid) is looked up in the young generation, then the old
// one; a hit writes MBFT_ACCEPT to status[i].  Every other item -- misses, slot
// words >= nslots (the host-decided kHostSlot | status words among them),
// invalid slots -- is appended, in no order, to e_c / r_c / s_c / slot_c with
// its index in origin; *miss (zeroed on st first by the caller) receives how
// many.  ndev (optional): the item count on the device; nothing at or past
// min(n, *ndev) is read or written.  force_hash (tests only, else null): item
// i's hash instead of memo_hash of its tuple.
struct MemoProbe {
  const uint8_t *e, *r, *s;
  const uint32_t* slot;
  long n;
  const uint32_t* ndev;
  const KeyDesc* keys;
  uint32_t nslots;
  const uint32_t* young;
  const uint32_t* old;
  uint64_t entries;
  uint8_t* status;
  uint8_t *e_c, *r_c, *s_c;
  uint32_t* slot_c;
  uint32_t* origin;
  uint32_t* miss;
  uint64_t* stats;
  const uint64_t* force_hash;
};
hipError_t memo_probe(const MemoProbe& p, hipStream_t st);
// k_memo_commit, one compacted item per lane, j < min(n, *miss):
// status[origin[j]] = status_c[j], and where that is MBFT_ACCEPT under a real
// valid key the tuple is inserted into the young generation: an empty entry of
// its probe sequence is claimed (0 -> busy by compare-and-swap), the payload
// written, the ready tag published behind an agent-scope release.  No empty
// entry in the sequence: the insert is dropped and counted, never an
// overwrite.  force_hash: per COMPACTED item.
struct MemoCommit {
  const uint8_t *e_c, *r_c, *s_c;
  const uint32_t* slot_c;
  const uint32_t* origin;
  const uint8_t* status_c;
  long n;
  const uint32_t* miss;
  const KeyDesc* keys;
  uint32_t nslots;
  uint32_t* young;
  uint64_t entries;
  uint8_t* status;
  uint64_t* stats;
  const uint64_t* force_hash;
};
hipError_t memo_commit(const MemoCommit& c, hipStream_t st);
// The key memory budget's ranking (key_rank.hip): every slot
// ranked on the GPU by its use count, one slot per lane, grid-stride on
// k_key_account's grid.  A slot's count u is the sum of its entry in the
// `nparts` (0 .. kRankParts) counter arrays of `part` -- one per engine, and
// the resident verifier's -- each of nslots entries; its bin is
// key_use_bin(u) (key_plan.h).  A LADDER slot is valid and its class is one of
// the nladder (1 .. kRankLadder) distinct codes of `ladder`, its rung the
// code's index.
constexpr int kRankParts = 4, kRankLadder = 8, kRankBins = 496;
struct KeyRank {
  const KeyDesc* keys;
  uint32_t nslots;
  int nparts;
  const uint64_t* part[kRankParts];
  int nladder;
  uint32_t ladder[kRankLadder];
};
// k_key_age: uses[i] >>= shift, rejects[i] >>= shift for i < n (shift 1 .. 63).
hipError_t key_age(uint64_t* uses, uint64_t* rejects, size_t n, unsigned shift, hipStream_t st);
// k_key_add: dst[i] += src[i] for i < n (counter arrays past kRankParts are
// added into one before the ranking).
hipError_t key_add(uint64_t* dst, const uint64_t* src, size_t n, hipStream_t st);
// k_key_hist: out[rung * kRankBins + bin] = the ladder slots of that rung and
// bin, out[kRankHistOutside] = the valid slots outside the ladder.  out
// (kRankHistWords words) is zeroed on st first.
constexpr int kRankHistOutside = kRankLadder * kRankBins, kRankHistWords = kRankHistOutside + 1;
hipError_t key_hist(const KeyRank& r, uint32_t* out, hipStream_t st);
// k_key_pick, plan mode: every ladder slot whose target rung,
// rung_of_bin[its bin] (kRankBins bytes on the device, each < nladder), differs
// from its rung is appended to list[target], in no order.  count[t] (kRankLadder
// words, zeroed on st first) receives how many belong on list t; only the first
// cap[t] of them are written.
struct KeyPickLists {
  uint32_t* list[kRankLadder];
  uint32_t cap[kRankLadder];
};
hipError_t key_pick_plan(const KeyRank& r, const uint8_t* rung_of_bin, const KeyPickLists& l, uint32_t* count,
                         hipStream_t st);
// k_key_pick, cold mode: the valid slots (of any class) with u <= max_uses,
// appended to list in no order, the first cap of them; *count (zeroed on st
// first) receives how many there are in all.
hipError_t key_pick_cold(const KeyRank& r, uint64_t max_uses, uint32_t* list, uint32_t cap, uint32_t* count,
                         hipStream_t st);
// MBFT_SPLIT_MAX (default 256; 0 disables the split form), read once.
long split_max_env();
hipError_t verify(const VerifyBatch& b, const VerifyTables& t, const mbft::VerifyPlan& plan, hipStream_t st);
// The inline-key form (k_verify_keys): n items whose keys
// stand beside them, xy n x 64 B big-endian X || Y, validated by the kernel.
// winv: 9 planes of n where the plan reads s^-1 from planes, else unused.  e,
// r, s and xy are 16-byte aligned.  Reads the generator table and nothing else.
struct KeysBatch {
  const uint8_t *e, *r, *s, *xy;
  long n;
  uint8_t* status;
  const uint32_t* winv;
};
// the device's compute units (what verify_keys_plan and the capped grids take)
int device_cus();
hipError_t verify_keys(const KeysBatch& b, const uint32_t* tabG, int wg, const mbft::KeysPlan& plan, hipStream_t st);
// The P-384 class (k_verify_p384, p384_kernels.hip): n items
// under keys that stand beside them, e, r, s n x 48 B and xy n x 96 B
// big-endian, all 16-byte aligned.  Reads nothing of any context.
struct P384Batch {
  const uint8_t *e, *r, *s, *xy;
  long n;
  uint8_t* status;
};
hipError_t verify_p384(const P384Batch& b, const mbft::P384Plan& plan, hipStream_t st);
// The resident verifier: one 256-thread workgroup per mailbox slot, or two
// (`two`: one per scalar, each on its own CU).
hipError_t verify_server(const mbft::ServerArgs& a, int servers, bool two, hipStream_t st);

}  // namespace mbft_launch
