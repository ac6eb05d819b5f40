/*
 * minbft_gpu.h -- C-ABI of the MI355X batch message authenticator for MinBFT.
 *
 * This is the drop-in boundary for MinBFT's message-authentication hot path.
 * Every entry point takes plain pointers and sizes, returns an integer code,
 * never throws, and never retains caller buffers after returning.
 *
 * What each entry point replaces in the reference (hyperledger-labs/minbft,
 * paths relative to the repository root):
 *
 *   mbft_ctx_create / mbft_add_role / mbft_set_public_key_* / mbft_enable_usig
 *       sample/authentication/authenticator.go:43-116 (New / NewWithSGXUSIG /
 *       NewWithUSIG / new: role -> scheme wiring) and
 *       sample/authentication/keymanager.go:179-227,352-366
 *       (LoadSimpleKeyStore, ecdsaKeySpec.parsePublicKey: x509 PKIX decode
 *       with on-curve validation).  Keys are validated and their comb tables
 *       precomputed on the GPU once (the replica set is static).
 *
 *   mbft_verify_message_authen_tag
 *       api/api.go:133-144 Authenticator.VerifyMessageAuthenTag, implemented
 *       by sample/authentication/authenticator.go:121-134 with the schemes
 *       sample/authentication/crypto.go:79-89,113-126 (ECDSA roles: digest =
 *       msg || SHA256(""), DER decode, crypto/ecdsa.Verify) and
 *       crypto.go:186-239 + usig/sgx/sgx-usig.go:81-101 +
 *       usig/sgx/usig-enclave.go:198-229 (USIG role: UI decode, epoch
 *       capture, SHA256(SHA256(msg)||epoch_le||counter_le), strict DER).
 *       Returns an mbft_status (>= 0) or an mbft_err (< 0).  MBFT_ACCEPT is
 *       Go's nil; MBFT_MALFORMED_DER in an ECDSA role is where Go panics
 *       (crypto.go:82-84); every other status is a Go error.
 *
 *   mbft_verify_batch
 *       NEW batch entry point (north_star item 1/2): n independent calls of
 *       the above, verified together on the GPU.  Results are exactly those
 *       of calling mbft_verify_message_authen_tag on items[0..n) in order:
 *       the USIG epoch capture (crypto.go:219-236) is replayed on the host in
 *       item order after the GPU has checked every signature.
 *
 *   mbft_generate_message_authen_tag
 *       api/api.go:143 GenerateMessageAuthenTag for the ECDSA roles
 *       (crypto.go:63-76,113-116: sign SHA256("")-suffixed digest, DER).
 *       The nonce is deterministic (RFC 6979-style) instead of crypto/rand;
 *       tags verify identically.  In the USIG role it creates one UI from the
 *       context's software USIG (mbft_usig_init, below) and is
 *       MBFT_ERR_STATE without one; tag_cap must then be at least
 *       MBFT_UI_SLOT.  The ECDSA roles' single call is
 *       NOT CONSTANT-TIME (the GPU signer, k_sign, gathers comb entries at
 *       addresses set by the nonce's digits): for tests and synthetic load
 *       only.  A production signer keeps the reference's CPU path (Go's
 *       constant-time P-256, crypto.go:63-76), as the Go binding does
 *       (go/gpuauth: GenerateMessageAuthenTag never calls the GPU).
 *
 *   mbft_generate_tags_prehashed / _flat / _prehashed_device,
 *   mbft_sign_messages_flat
 *       NEW batch form of the same GenerateMessageAuthenTag for the ECDSA
 *       roles, fit for real keys: a second signer (k_sign_tags) whose memory
 *       addresses, branches and loop counts do not depend on the key or the
 *       nonce, RFC 6979 nonces, DER on the device.  What the core signs per
 *       executed request (REPLY: core/utils.go:43-53,
 *       core/message-handling.go:552-568) and the client per request
 *       (client/request.go:194-204).
 *
 *   mbft_verify_prehashed / mbft_verify_prehashed_device
 *       Go crypto/ecdsa.Verify(pub, hash, r, s) as called at
 *       sample/authentication/crypto.go:86 and
 *       usig/sgx/usig-enclave.go:224, for a batch of already-decoded
 *       (e, r, s, key slot) items.  The _device variant takes device
 *       pointers and an hipStream_t (as void*) and is what bench.py times.
 *
 *   mbft_der_parse_sig
 *       encoding/asn1.Unmarshal(sig, &struct{R, S *big.Int}) as used at
 *       crypto.go:81 and usig-enclave.go:217 (host-only, no GPU needed).
 */
#ifndef MINBFT_GPU_H
#define MINBFT_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Per-item verification outcome (also the value returned by
 * mbft_verify_message_authen_tag). */
enum mbft_status {
  MBFT_ACCEPT = 0,         /* Go: nil */
  MBFT_REJECT_SIG = 1,     /* ecdsa.Verify false: r/s range, infinity, x mismatch */
  MBFT_MALFORMED_DER = 2,  /* asn1.Unmarshal error (ECDSA roles: Go panics) */
  MBFT_DER_TRAILING = 3,   /* USIG: "extra bytes in USIG signature" */
  MBFT_UNKNOWN_KEY = 4,    /* known role, no key for this id (pk == nil) */
  MBFT_BAD_KEY = 5,        /* key slot invalid (never reachable from Go) */
  MBFT_BAD_UI = 6,         /* USIG tag shorter than 8 bytes (usig.go:75-80) */
  MBFT_BAD_CERT = 7,       /* USIG cert shorter than 8 bytes (sgx-usig.go:159-168) */
  MBFT_ZERO_COUNTER = 8,   /* core/usig-ui.go:65-67 (core-level check) */
  MBFT_EPOCH_MISMATCH = 9, /* sgx-usig.go:92-94 */
  MBFT_UNKNOWN_ROLE = 10   /* keymanager.go:100, authenticator.go:126-129 */
};

/* Return codes of API calls (negative). */
enum mbft_err {
  MBFT_OK = 0,
  MBFT_ERR_ARG = -1,
  MBFT_ERR_HIP = -2,
  MBFT_ERR_NOMEM = -3,
  MBFT_ERR_KEY = -4,     /* invalid / off-curve public key (x509 parse error) */
  MBFT_ERR_STATE = -5,   /* e.g. signing without a private key */
  MBFT_ERR_NODEV = -6    /* no usable GPU */
};

/* api/api.go:98-115 AuthenticationRole */
enum mbft_role { MBFT_ROLE_REPLICA = 1, MBFT_ROLE_USIG = 2, MBFT_ROLE_CLIENT = 3 };

typedef struct mbft_ctx mbft_ctx;

/* One authenticator call for mbft_verify_batch. */
typedef struct mbft_item {
  uint32_t role;
  uint32_t id;
  const uint8_t* msg;
  size_t msg_len;
  const uint8_t* tag;
  size_t tag_len;
} mbft_item;

int mbft_version(void);
int mbft_device_count(void);

/* Context = one authenticator.  Created on one GPU (builds the generator
 * comb table there); mbft_ctx_add_device adds an engine on another GPU of
 * the node (or the same one: more streams), which receives replicas of the
 * generator and every key table, now and for keys registered later.  The
 * host-buffer entry points (mbft_verify_batch, mbft_verify_message_authen_tag,
 * mbft_verify_prehashed, mbft_validate_messages) then split each batch into
 * contiguous shards of at least mbft_set_shard_min items (default 32768),
 * one host thread, HIP stream and device per engine, with no collective:
 * only each shard's status bytes come back, in index order, and the USIG
 * epoch replay runs afterwards on the host.  The *_device entry points run
 * on the creating device only.  mbft_ctx_devices returns the engine count
 * and fills devices[0..cap).  (Multi-process, one GPU per process, is the
 * other multi-GPU model: bench.py and DESIGN.md §7.) */
int mbft_ctx_create(int device, mbft_ctx** out);
void mbft_ctx_destroy(mbft_ctx* ctx);
const char* mbft_last_error(const mbft_ctx* ctx);
int mbft_ctx_add_device(mbft_ctx* ctx, int device);
int mbft_ctx_devices(const mbft_ctx* ctx, int* devices, int cap);
int mbft_set_shard_min(mbft_ctx* ctx, size_t items);

/* Key store.  A role exists once declared (even with no keys).  Public keys
 * are 91-byte PKIX DER (keymanager.go:352-366) or raw 64-byte X||Y. */
int mbft_add_role(mbft_ctx* ctx, uint32_t role);
int mbft_set_public_key_pkix(mbft_ctx* ctx, uint32_t role, uint32_t id, const uint8_t* pkix,
                             size_t len);
int mbft_set_public_key_xy(mbft_ctx* ctx, uint32_t role, uint32_t id, const uint8_t xy[64]);
/* Registers raw points without the role/id mapping; out_slots receive key
 * slots for mbft_verify_prehashed*.  valid_out[i] = 1 if on-curve. */
int mbft_register_points(mbft_ctx* ctx, const uint8_t* xy64, size_t n, uint32_t* out_slots,
                         uint8_t* valid_out);
/* Drops every key: all (role, id) -> key mappings, all slots and their comb
 * tables, and the USIG epoch state; declared roles stay.  The tables' device
 * blocks are kept for reuse by the next registrations (re-mapping 129 GiB
 * takes seconds) and released when the generator table is rebuilt, when an
 * allocation would otherwise fail, and at destroy.  Equivalent to
 * building the authenticator again over a new key store
 * (keymanager.go:179-227 LoadSimpleKeyStore + authenticator.go:88-116).
 * Waits for in-flight work. */
int mbft_clear_keys(mbft_ctx* ctx);
/* Slot of (role, id), or MBFT_ERR_KEY if absent. */
int mbft_key_slot(const mbft_ctx* ctx, uint32_t role, uint32_t id);
/* Comb windows.  Signed digits: a window of W bits costs
 * ceil(256/W) table entries per scalar and about ceil(256/W) x 2^(W-1) x
 * 64 B of HBM per table:
 *   W =  8: 32 entries, 0.25 MiB      W = 24: 11 entries, 5.0 GiB
 *   W = 16: 16 entries, 34 MiB        W = 26: 10 entries, 18.3 GiB
 *   W = 22: 12 entries, 1.4 GiB       W = 29:  9 entries, 129 GiB
 * (the last window's table is cut to the digits a 256-bit scalar reaches).
 * mbft_set_key_window sets the window for keys registered AFTER the call
 * (default 16); a single static signer fits at W = 29 next to a W = 29
 * generator table (258 GiB of 288), a 33-replica set at W = 24, a very
 * large client set at W = 8.  mbft_set_generator_window rebuilds the shared
 * generator table (default 16); it waits for in-flight work.
 * Both accept 4 <= W <= 29; MBFT_ERR_NOMEM if the table does not fit.
 *
 * mbft_set_key_window also accepts MBFT_WINDOW_NONE (0): keys registered
 * after the call are TABLE-FREE.  Such a key costs 64 bytes of HBM (its point,
 * in pooled blocks) and registers at the price of the on-curve check: no
 * table build.  A signature under it is verified by a double-and-add ladder
 * over the point instead of a comb -- about 2,900 field reductions an item
 * against about 170 at W = 29, so far slower per item, but for any number of
 * keys and from the moment a key is first seen.  Meant for open or very
 * large client sets; every verify entry point serves such keys, and keys of
 * every window, 0 included, live side by side in one context.  The generator
 * always has a table: mbft_set_generator_window(ctx, 0) is MBFT_ERR_ARG, as
 * are the windows 1..3 for both.  mbft_get_windows reports 0 while it is set. */
#define MBFT_WINDOW_NONE 0
int mbft_set_key_window(mbft_ctx* ctx, int wbits);
int mbft_set_generator_window(mbft_ctx* ctx, int wbits);
int mbft_get_windows(const mbft_ctx* ctx, int* g_wbits, int* q_wbits);
/* COMPACT keys: between the table-free class (64 B a key) and the smallest
 * comb window (32 KiB a key at W = 4).  mbft_set_key_teeth(ctx, t), t in
 * MBFT_TEETH_MIN .. MBFT_TEETH_MAX, gives keys registered AFTER the call a
 * small table of 2^t entries of 64 B (in pooled blocks), verified by a comb
 * WITH doublings (Lim-Lee): d = ceil(256 / t) columns, d - 1 doublings and at
 * most d additions a signature.  Memory per key and field reductions for
 * u2 Q, counted from the formulas (doubling 8, mixed addition 10), against
 * about 2,900 for the table-free ladder and about 170 for a whole W = 29
 * verify:
 *   t = 2: 256 B, ~1,980 (0.68 of the ladder)   t = 6:  4 KiB, ~760 (0.26)
 *   t = 3: 512 B, ~1,430 (0.49)                 t = 8: 16 KiB, ~570 (0.20)
 *   t = 4: 1 KiB, ~1,100 (0.38)
 * A million clients at t = 4 take 1 GiB.  DESIGN.md §4.8 has the measured
 * rates.  Any other t is MBFT_ERR_ARG; MBFT_ERR_NOMEM at registration if the
 * tables do not fit (the slots stay invalid).  A later mbft_set_key_window
 * -- MBFT_WINDOW_NONE included -- switches back to windows; its accepted
 * range is what it was.  While teeth are selected mbft_get_windows reports
 * key window 0 and mbft_get_key_teeth reports t; mbft_get_key_teeth reports
 * 0 while the current class is a window.  Every verify entry point serves
 * such keys (the resident verifier hands them to the ordinary path), and
 * keys of every class -- windows 4..29, window 0, teeth 2..8 -- live side by
 * side in one context. */
#define MBFT_TEETH_MIN 2
#define MBFT_TEETH_MAX 8
int mbft_set_key_teeth(mbft_ctx* ctx, int teeth);        /* keys registered AFTER the call */
int mbft_get_key_teeth(const mbft_ctx* ctx, int* teeth); /* 0 while the current class is a window */
/* SIGNED COMPACT keys: the same comb over a signed all-nonzero recoding of
 * u2, whose table holds only the entries with a positive top tooth: 2^(t-1)
 * entries of 64 B for t teeth, half the compact table of the same t -- one
 * more tooth for the same bytes.  mbft_set_key_signed_teeth(ctx, t), t in
 * MBFT_STEETH_MIN .. MBFT_STEETH_MAX, gives keys registered AFTER the call
 * this class.  Bytes per key and field reductions for u2 Q, counted from the
 * formulas (doubling 8, mixed addition 10; the signed comb has no zero
 * column, d - 1 doublings and d - 1 additions):
 *   bytes/key   unsigned        signed         ratio
 *   128 B       -- (ladder, 64 B: ~2,900)  s2: 2,286   new point
 *   256 B       t2: ~1,980      s3: 1,530      0.77
 *   512 B       t3: ~1,430      s4: 1,134      0.79
 *   1 KiB       t4: ~1,100      s5:   918      0.83
 *   2 KiB       t5:   ~912      s6:   756      0.83
 *   4 KiB       t6:   ~760      s7:   648      0.85
 *   8 KiB       t7:   ~655      s8:   558      0.85
 *   16 KiB      t8:   ~570      s9:   504      0.88
 * A million clients at 4 signed teeth take 512 MiB.  These are counts;
 * measured, signed t runs in the time of unsigned t at half
 * its bytes, and at equal bytes in 0.71 (s3 / t2) to 0.95 (s9 / t8) of the
 * unsigned class's time: faster for every t.  Any other t is MBFT_ERR_ARG; MBFT_ERR_NOMEM at registration
 * if the tables do not fit (the slots stay invalid).  mbft_set_key_teeth and
 * mbft_set_key_window switch away from this class as they switch between
 * each other.  While signed teeth are selected mbft_get_windows reports key
 * window 0, mbft_get_key_teeth reports 0 and mbft_get_key_signed_teeth
 * reports t (0 while another class is selected).  Every verify entry point
 * serves such keys, side by side with every other class. */
#define MBFT_STEETH_MIN 2
#define MBFT_STEETH_MAX 9
int mbft_set_key_signed_teeth(mbft_ctx* ctx, int teeth);        /* keys registered AFTER the call */
int mbft_get_key_signed_teeth(const mbft_ctx* ctx, int* teeth); /* 0 unless this class is selected */
/* THE LIFE OF A KEY AFTER REGISTRATION.  Every call below
 * that changes the key store waits for the library's batches in flight, like
 * registration, and is replayed on the peer engines (mbft_ctx_add_device).
 *
 * A key's CLASS has one code, the one its descriptor carries: a comb window
 * 4..29, MBFT_WINDOW_NONE (table-free), MBFT_KEY_CLASS_TEETH(t) for a
 * compact key of t = MBFT_TEETH_MIN..MBFT_TEETH_MAX teeth, or
 * MBFT_KEY_CLASS_SIGNED_TEETH(t) for a signed compact key of t =
 * MBFT_STEETH_MIN..MBFT_STEETH_MAX teeth.  Classes are ordered by the bytes
 * of one key's data (64 B, 64 B x 2^t, 64 B x 2^(t-1), the comb table); a
 * signed t and an unsigned t - 1 tie, and neither is promoted into the other.
 *
 * Use counts.  mbft_set_key_accounting(ctx, 1) (default off: nothing is
 * allocated, no batch launches anything more) makes every batch end with one
 * more kernel on its stream that adds, per key slot, `uses` -- the batch's
 * items whose slot is registered and valid -- and `rejects` -- those of them
 * whose status is not MBFT_ACCEPT -- into 64-bit counters on the GPU, one pair
 * per slot and engine.  NOT counted, because no slot can be charged: items the
 * host decided before the signature check (unknown role or id, malformed tag,
 * ...), items whose slot number is not registered, and items under an invalid
 * or released slot.  The counts are VERIFIES PERFORMED, not calls received: the
 * message layer verifies identical calls once and counts them once.  Single
 * calls served by the resident verifier are counted on the host and merged
 * when the counts are read.  Sharded batches are counted shard by shard.
 *   mbft_key_usage: uses_out[i] / rejects_out[i] (either may be NULL) of
 *     slots[i], or of slot i when slots is NULL, summed over the engines and
 *     the resident counter; 0 for a slot that does not exist.  It waits for the
 *     library's batches and synchronizes the library's own streams; work a
 *     caller queued on a stream of its own (mbft_verify_prehashed_device) is
 *     counted once that stream has finished -- synchronize it first.
 *   mbft_reset_key_usage: every counter back to zero (synchronizes the
 *     device).  A released slot's counters are zeroed; mbft_clear_keys zeroes
 *     all.  Counters live for the context, not across processes.
 *
 * Re-classing.  mbft_set_key_class rebuilds the verification data of the
 * registered key (role, id) in class cls; mbft_set_slot_classes does it for n
 * slots at once.  The new data is built first, then the descriptors are
 * swapped, then the old storage is released: on MBFT_ERR_NOMEM or any other
 * failure the keys keep their class and go on verifying.  Slots already in cls
 * are skipped; an unknown class code is MBFT_ERR_ARG; an invalid slot is
 * MBFT_ERR_ARG in the single form and skipped in the bulk form (a slot number
 * that does not exist is MBFT_ERR_ARG in both).  Each call that changes
 * anything costs ONE device synchronize per engine (the resident verifier is
 * parked first), whatever n is: the bulk form exists to share it.  Use counts
 * are kept.
 *   mbft_get_key_class: the class of (role, id) and the bytes of its data.
 *   mbft_promote_hot_keys: of the valid keys whose class is cheaper in memory
 *     than cls and whose uses are >= min_uses, the max_keys with the most uses
 *     (ties: the lower slot) are re-classed into cls in one bulk call;
 *     *promoted receives how many were chosen.
 *
 * Removal.  mbft_remove_public_key unmaps (role, id) (MBFT_ERR_KEY when it is
 * not mapped): the pair then reads MBFT_UNKNOWN_KEY through every entry point,
 * like an id never registered, and may be registered again, with the same or
 * another key.  A slot is RELEASED when no (role, id) maps to it any more and
 * its number was not handed out by mbft_register_points; mbft_release_slots
 * gives that claim up (and releases the slots nothing maps to).  A released
 * slot is invalid -- device entry points that still name it read MBFT_BAD_KEY
 * -- its number is taken first, lowest first, by the next registration, and
 * its storage by the next single-key registration or re-class of its class,
 * so neither the descriptor array nor the key blocks grow under churn.  A call
 * that releases slots costs one device synchronize per engine.  Mapping a
 * registered pair to ANOTHER key with mbft_set_public_key_* (rotation by
 * overwriting) releases the pair's earlier slot under the same rule, at the
 * same cost.
 *   mbft_key_memory: out[0] bytes of live key data, out[1] bytes of released
 *     pieces awaiting reuse, out[2] bytes of key blocks held, on the
 *     context's own engine. */
#define MBFT_KEY_CLASS_TEETH(t) (0x100 | (t))
#define MBFT_KEY_CLASS_SIGNED_TEETH(t) (0x200 | (t))
int mbft_set_key_accounting(mbft_ctx* ctx, int enabled);
int mbft_key_usage(mbft_ctx* ctx, const uint32_t* slots, size_t n, uint64_t* uses_out,
                   uint64_t* rejects_out);
int mbft_reset_key_usage(mbft_ctx* ctx);
int mbft_get_key_class(const mbft_ctx* ctx, uint32_t role, uint32_t id, uint32_t* cls,
                       uint64_t* table_bytes);
int mbft_set_key_class(mbft_ctx* ctx, uint32_t role, uint32_t id, uint32_t cls);
int mbft_set_slot_classes(mbft_ctx* ctx, const uint32_t* slots, size_t n, uint32_t cls);
int mbft_promote_hot_keys(mbft_ctx* ctx, uint32_t cls, size_t max_keys, uint64_t min_uses,
                          size_t* promoted);
int mbft_remove_public_key(mbft_ctx* ctx, uint32_t role, uint32_t id);
int mbft_release_slots(mbft_ctx* ctx, const uint32_t* slots, size_t n);
int mbft_key_memory(const mbft_ctx* ctx, uint64_t out[3]);
/* THE KEY MEMORY BUDGET.  The calls below follow the rules
 * above: they wait for the library's batches in flight, are replayed on the
 * peer engines, synchronize the library's own streams before the counters are
 * read, and count work on a caller's own stream once that stream has finished.
 * With no budget set and none of them called nothing is allocated or launched.
 *   mbft_age_key_usage: every counter of every engine, and the resident
 *     verifier's counts, shifted right by `shift` bits, so that old use fades.
 *     0 does nothing; >= 64 is MBFT_ERR_ARG.  Each engine's counter is shifted
 *     on its own: with P of them a slot's sum lands in
 *     [(total >> shift) - (P - 1), total >> shift].
 *   mbft_set_key_budget / mbft_get_key_budget: the bytes of LIVE KEY DATA PER
 *     ENGINE (mbft_key_memory's out[0]) that mbft_rebalance_keys plans
 *     against; 0, the default, is none.  Registration is never refused for the
 *     budget's sake.
 *   mbft_key_class_cost: the MODELLED field reductions of u2 Q under a key of
 *     class cls -- 10 ceil(256 / W) for a comb window W, 2,908 table-free,
 *     18 ceil(256 / t) - 8 for t teeth, signed or not; a model, not a
 *     measurement.  0 for an unknown code.
 *   mbft_rebalance_keys: gives every key whose class is a rung of `ladder` the
 *     rung of its use count, so that the modelled verify cost is lowest within
 *     the budget; it demotes and promotes.  `ladder`: 1 .. 8 class codes,
 *     bytes strictly ascending, cost strictly descending, the gain per byte of
 *     each step strictly decreasing (a dominated or non-convex rung is
 *     MBFT_ERR_ARG).  The plan: every ladder key starts at rung 0; keys are
 *     binned by use count (exact below 16, then eight bins an octave) and a
 *     whole bin moves up one rung at a time, the steps taken in descending
 *     order of (the bin's least count) x (reductions saved per byte) while the
 *     bytes fit, stopping at the first step that does not fit; bins whose least
 *     count is below max(min_uses, 1) stay at rung 0.  The budget may be left
 *     unused by less than that step's bytes.  Valid keys of any other class are
 *     PINNED: they keep their class and their bytes count against the budget.
 *     Demotions are applied first, one bulk re-class per target rung from rung
 *     0 upwards, then promotions from the top rung downwards, which reuse the
 *     storage the demotions released; each non-empty bulk step costs one device
 *     synchronize per engine.  A failure (MBFT_ERR_NOMEM, ...) stops the walk:
 *     every bulk step is all or nothing, keys not yet moved keep their class,
 *     *out reports what was done.  Where even rung 0 for every ladder key
 *     exceeds the budget that plan is applied all the same and the call
 *     returns MBFT_OK with over_budget set.  Use counts are kept.
 *     MBFT_ERR_STATE: accounting is off (all-zero counts would demote every
 *     key), or no budget is set.
 *   mbft_cold_keys: the valid slots, of any class, whose summed uses are <=
 *     max_uses, ascending -- the `cap` lowest when there are more -- and in
 *     *count how many there are in all.  It changes nothing: eviction stays
 *     the caller's (mbft_remove_public_key, mbft_release_slots). */
typedef struct mbft_rebalance_result {
  uint64_t live_before, live_after; /* mbft_key_memory's out[0] */
  uint64_t pinned_bytes;            /* valid keys outside the ladder */
  uint64_t over_budget;             /* bytes past the budget with every ladder key at rung 0, else 0 */
  uint32_t promoted, demoted;       /* keys moved up / down */
  uint32_t keys_per_rung[8];        /* afterwards */
} mbft_rebalance_result;
int mbft_age_key_usage(mbft_ctx* ctx, unsigned shift);
int mbft_set_key_budget(mbft_ctx* ctx, uint64_t bytes);
int mbft_get_key_budget(const mbft_ctx* ctx, uint64_t* bytes);
uint32_t mbft_key_class_cost(uint32_t cls);
int mbft_rebalance_keys(mbft_ctx* ctx, const uint32_t* ladder, size_t nladder, uint64_t min_uses,
                        mbft_rebalance_result* out);
int mbft_cold_keys(mbft_ctx* ctx, uint64_t max_uses, uint32_t* slots_out, size_t cap, size_t* count);
/* The verified-call memo: accepted signature checks
 * remembered across batches.  MinBFT validates nested messages -- a COMMIT
 * re-validates its embedded PREPARE (core/commit.go:82), the PREPARE its
 * embedded REQUEST (core/prepare.go:55) -- so a backup makes 3n - 3
 * authenticator calls a request of which n are distinct (SURVEY section 8(f)
 * row 2, Appendix B), and the copies arrive in different batches.  The result
 * of a signature check is a pure function of (key, e, r, s): with the memo on,
 * the message layer's device passes (mbft_check_messages* / mbft_validate_
 * messages* past the small route) look every unique call up in a table of
 * accepted (key slot, e, r, s) tuples in device memory; a hit is accepted
 * without running the check, only the misses go to the verifier, and the
 * accepted misses are then remembered.  Only accepts are remembered.  Every hit
 * is confirmed by comparing the whole tuple.
 *   What the memo does NOT change: any status or reject kind, the USIG epoch
 *   step (applied per check afterwards, as before: e holds the epoch and the
 *   counter, the step is not part of the tuple), where a stream stops, the
 *   per-key use counts.  Off (the default), no kernel of it is launched.
 *   mbft_set_verified_memo: `bytes` of device memory on every engine for the
 *     table, rounded down to two generations of a power-of-two number of
 *     128-byte entries (at least 2 x 1,024: MBFT_ERR_ARG below); 0 turns the
 *     memo off and frees it.  Setting it again starts empty.  MBFT_ERR_NOMEM
 *     leaves the previous state in place.
 *   mbft_get_verified_memo: the rounded size in use (0: off).
 *   mbft_verified_memo_stats: lookups, hits, inserts, dropped (inserts that
 *     found their probe window full), rotations, clears, summed over the
 *     engines; lookups - hits is what went to the verifier.
 *   mbft_clear_verified_memo: forget everything.  The library does so itself
 *     whenever a slot number can come to mean another point
 *     (mbft_remove_public_key, mbft_release_slots, mbft_clear_keys);
 *     re-classing, promotion and mbft_rebalance_keys keep the point and the
 *     memo. */
int mbft_set_verified_memo(mbft_ctx* ctx, uint64_t bytes);
int mbft_get_verified_memo(mbft_ctx* ctx, uint64_t* bytes);
int mbft_verified_memo_stats(mbft_ctx* ctx, uint64_t out[6]);
int mbft_clear_verified_memo(mbft_ctx* ctx);
/* USIG scheme present (authenticator.go:102-110: absent without a USIG). */
int mbft_enable_usig(mbft_ctx* ctx, int enabled);
/* Private key for GenerateMessageAuthenTag in an ECDSA role. */
int mbft_set_private_key(mbft_ctx* ctx, uint32_t role, const uint8_t d[32]);

/* api.Authenticator */
int mbft_verify_message_authen_tag(mbft_ctx* ctx, uint32_t role, uint32_t id,
                                   const uint8_t* msg, size_t msg_len, const uint8_t* tag,
                                   size_t tag_len);
int mbft_verify_batch(mbft_ctx* ctx, const mbft_item* items, size_t n, uint8_t* status_out);
/* Coalescing of concurrent single calls (new; the reference's ECDSA scheme
 * is called from many goroutines at once, api/api.go:132).  When enabled,
 * mbft_verify_message_authen_tag calls that arrive while the batch slots are
 * busy are queued and verified together as the next batch (group commit):
 * one batch at a time (mbft_set_coalescing_slots: up to that many), the
 * first queued caller without a slot leads the next one, every caller gets
 * its own status, and each batch keeps the queue's order (the USIG epoch step
 * runs in that order --
 * concurrent callers have no order of their own, as under the reference's
 * mutex, crypto.go:215-218).  max_wait_us > 0 also lets a leader wait that
 * long for company when it would otherwise run alone; 0 adds no latency.
 * max_batch caps a batch (0: no cap).  Default: disabled (each call is its
 * own GPU round trip). */
int mbft_set_coalescing(mbft_ctx* ctx, int enabled, uint32_t max_wait_us, uint32_t max_batch);
/* Coalesced batches in flight at once (new): 1..64, default 1; at most the
 * mbft_set_concurrency lanes are used (each batch runs on a lane). */
int mbft_set_coalescing_slots(mbft_ctx* ctx, int slots);
/* The resident single-call verifier (new; replaces, for
 * mbft_verify_message_authen_tag, the per-call kernel launch behind
 * api/api.go:133-144 / sample/authentication/authenticator.go:121-134).
 * slots 1..64: a verify kernel stays on the GPU while calls keep arriving:
 * mailbox slots in host-mapped memory served by a pool of 256-thread
 * workgroups (2 per slot up to MBFT_RESIDENT_SERVERS, default 16); a call
 * takes a free slot, runs its host part (role, DER, digest, key, s^-1),
 * posts the item and sleeps through its expected GPU time, then waits on its
 * done words -- no launch, no stream synchronize, and concurrent callers (up
 * to `slots`) never wait for each other's batch.  The kernel leaves after MBFT_RESIDENT_IDLE_US (default
 * 2000) without a call or MBFT_RESIDENT_LIFE_MS (default 200) after its
 * start, and the next call relaunches it (a relaunch under batch load waits
 * for CUs: at 20 ms a trickle's p99 was ~200 us, at 200 ms 32-51 us).  A
 * device-wide synchronize of the application waits for the live generation;
 * the library's own batch paths make none.  Calls past `slots` at once take
 * the coalescer / batch path.  Statuses, USIG epoch step and errors are those
 * of the other paths.  0 (default) turns it off; waits for calls in flight. */
int mbft_set_resident(mbft_ctx* ctx, int slots);
/* out[6]: slots, calls served, kernel launches, calls that found every slot
 * taken, relaunches found by a stream query, 1 if the kernel's stream has
 * its own hardware queue (the lowest stream priority, which no other stream
 * of the library uses). */
int mbft_resident_stats(mbft_ctx* ctx, double out[6]);
/* out[5] (new, round 6): the caller-side wait of resident calls -- sleeps
 * taken, sleeps that woke after the items were done, the current estimates
 * (ns) of a lone item's post -> done time and of a sleep's wake-up delay,
 * and 1 if the wait sleeps (MBFT_RESIDENT_SLEEP, default 1) or 0 if it spins.
 * The CPU a call costs its caller is its host part, the join, the wake-up and
 * the last spin, not the GPU time (the reference verifies on the calling
 * goroutine's CPU, api/api.go:132, sample/authentication/crypto.go:79-89). */
int mbft_resident_wait_stats(mbft_ctx* ctx, double out[5]);
/* Test hook (new, round 6): host threads the library has started so far
 * (worker pools, one shard thread per engine).  A batch on a multi-engine
 * context starts none once its engines are warm (one host
 * thread per GPU, persistent). */
uint64_t mbft_debug_threads_started(void);
/* Test hook (new): the host end of a resident-kernel verify -- nparts (1..16)
 * partial comb sums in the device's limb format (40 words each: X, Y, ZZ, ZZZ
 * as 9 29-bit Montgomery limbs, then a flags word, 1 = infinity) joined and
 * x-checked against r (32 B big-endian).  0 accept, 1 reject. */
int mbft_debug_host_join(const uint32_t* part, int nparts, const uint8_t* r_be);
/* Test hook (new): a resident call's scalars as the host computes them for the
 * kernel (SrvSlot::u) -- u1 = e s^-1, u2 = r s^-1 mod N, 8 little-endian words
 * each, from e, r, s (32 B big-endian each); zeros when s is 0 or >= N.
 * crypto/ecdsa.Verify's u1, u2 (sample/authentication/crypto.go:86). */
int mbft_debug_host_scalars(const uint8_t* e, const uint8_t* r, const uint8_t* s, uint32_t u[16]);
/* Concurrent batches on one GPU (new; the reference calls the authenticator
 * from every peer's and client's stream goroutine at once, api/api.go:132).
 * With lanes > 1, up to `lanes` calls of mbft_verify_batch{,_flat},
 * mbft_check_batch{,_flat} and mbft_verify_message_authen_tag run at the
 * same time: each leases a lane (its own staging, device scratch, streams,
 * s^-1 pipeline and host workers) and shares the context's tables and key
 * store, so their copies and kernels overlap on the device.  The USIG epoch
 * step of a verify batch is applied under the context's lock, one batch at
 * a time, each batch in its own call order -- the outcome of some sequential
 * order of the concurrent calls, as under the reference's scheme lock
 * (crypto.go:198-199).  Key, role and window changes wait for the batches in
 * flight.  Every other entry point keeps running one at a time.  lanes = 1
 * (default) serialises every call on the context.  1 <= lanes <= 64. */
int mbft_set_concurrency(mbft_ctx* ctx, int lanes);
int mbft_get_concurrency(const mbft_ctx* ctx);
/* Comb windows planned from the device's free HBM and the key counts per
 * role (new; what the Go binding uses when no window is configured):
 * greedy over the upgrades with the most table additions saved per verify
 * per byte (a key class weighted by its share of a replica's verifies:
 * ~n USIG UIs and one client signature per request), leaving 6 GiB for
 * batch scratch.  One static signer gets 29 / 29; 33 USIG keys and a
 * client get a generator and key windows that fit together. */
int mbft_plan_windows(int device, size_t n_replica, size_t n_usig, size_t n_client, int* g_wbits,
                      int* replica_wbits, int* usig_wbits, int* client_wbits);
/* mbft_verify_batch over flat buffers: call i = (roles[i], ids[i],
 * msgs[msg_off[i] .. msg_off[i+1]), tags[tag_off[i] .. tag_off[i+1])).  No
 * pointers inside the arguments, so Go can pass its own slices (cgo forbids
 * Go pointers stored in C memory, which an mbft_item array would need). */
int mbft_verify_batch_flat(mbft_ctx* ctx, const uint32_t* roles, const uint32_t* ids,
                           const uint8_t* msgs, const uint64_t* msg_off, const uint8_t* tags,
                           const uint64_t* tag_off, size_t n, uint8_t* status_out);
/* The compact flat form (new): the same calls with 1-byte roles and 32-bit
 * offsets (a batch's message and tag bytes each below 4 GiB).  With the
 * buffers in library page-locked memory a call crosses PCIe in 13 bytes plus
 * its message and tag instead of 24 plus them.  For the ECDSA roles the
 * verdict depends on the message only through e = (msg || SHA256(""))[0:32]
 * (crypto.go:113-126: Sum(m) appends the empty digest, Verify reads 32
 * bytes), so a caller may pass those 32 bytes as the message -- copied, not
 * hashed -- and the statuses are the same (the Go binding does: 32 B instead
 * of 47 for a REQUEST).  Offsets are checked where they are read: with the
 * device decode each call's fields must lie in the batch's byte ranges in
 * order, else MBFT_ERR_ARG (statuses unspecified, no state changed). */
int mbft_verify_batch_flat32(mbft_ctx* ctx, const uint8_t* roles, const uint32_t* ids,
                             const uint8_t* msgs, const uint32_t* msg_off, const uint8_t* tags,
                             const uint32_t* tag_off, size_t n, uint8_t* status_out);
/* Library-owned page-locked host memory (new).  When EVERY buffer of a
 * mbft_verify_batch_flat / mbft_check_batch_flat call (roles, ids, msg_off,
 * tag_off, and the used ranges of msgs and tags) lies in such allocations,
 * the calls travel to the GPU raw, chunk by chunk, and are decoded there
 * (role / key dispatch, Go-exact DER, the Sum(m) digest, the USIG UI / cert
 * split and digest chain; prep_kernels.hip k_prepare): the host reads none of
 * their bytes except the roles (a scan for USIG calls, whose epoch step
 * stays on the host in call order).  Results are identical to the host
 * decode.  A status_out in such memory also receives the statuses straight
 * from the GPU.  The Go binding marshals its batches into these buffers
 * (cgo: C memory).  mbft_host_alloc: MBFT_ERR_NOMEM on failure;
 * mbft_host_free: MBFT_ERR_ARG for a pointer it did not return. */
int mbft_host_alloc(size_t bytes, void** out);
int mbft_host_free(void* p);
/* Device decode on (1, default) or off (0: always the host decode). */
int mbft_set_device_prepare(mbft_ctx* ctx, int enabled);
/* Kernel for batches below the batched-s^-1 threshold (new; tuning and
 * tests): up to split_max items take k_verify_split (one item per 4-wave
 * workgroup, the comb windows split over the waves: the lowest latency for
 * single calls, s^-1 per wave), larger ones the lane-pair / lane-quad
 * kernels (mbft_set_small_batch_inverse).
 * split_max < 0: env MBFT_SPLIT_MAX, default 256; 0: pairs only. */
int mbft_set_small_batch_form(mbft_ctx* ctx, long split_max);
/* The form of the small batches past the split kernel's (new; tuning and
 * tests): 2 k_verify_quads (an item per lane quad, each lane half of one
 * scalar's windows) with s^-1 by each wave inside it (one wave-cooperative
 * inversion per 16 items); 3 the batched per-wave s^-1 into planes first
 * (k_ninv_local), then k_verify_quads; 1 the planes, then k_verify_pairs (an
 * item per lane pair); 0 k_verify_pairs inverting s per lane (divsteps); -1
 * the default (2).
 * MBFT_ERR_ARG outside -1..3. */
int mbft_set_small_batch_inverse(mbft_ctx* ctx, int mode);
/* Two-phase form of the same semantics, for callers that must keep their
 * own per-call order (the core's stream loops):
 *   mbft_check_batch   the pure part of n calls, all signatures on the GPU
 *                      at once, NO state touched: pure_out[i] = the status
 *                      call i gets if its USIG epoch check passes;
 *   mbft_resolve_checked  later, per call and in call order: the host part
 *                      of the call again plus the USIG epoch step
 *                      (crypto.go:219-236) over `pure` -- no GPU work.
 * resolve_checked(call, check(call)) == verify_message_authen_tag(call). */
int mbft_check_batch(mbft_ctx* ctx, const mbft_item* items, size_t n, uint8_t* pure_out);
int mbft_check_batch_flat(mbft_ctx* ctx, const uint32_t* roles, const uint32_t* ids,
                          const uint8_t* msgs, const uint64_t* msg_off, const uint8_t* tags,
                          const uint64_t* tag_off, size_t n, uint8_t* pure_out);
int mbft_check_batch_flat32(mbft_ctx* ctx, const uint8_t* roles, const uint32_t* ids,
                            const uint8_t* msgs, const uint32_t* msg_off, const uint8_t* tags,
                            const uint32_t* tag_off, size_t n, uint8_t* pure_out);
int mbft_resolve_checked(mbft_ctx* ctx, uint32_t role, uint32_t id, const uint8_t* msg,
                         size_t msg_len, const uint8_t* tag, size_t tag_len, uint8_t pure);
int mbft_generate_message_authen_tag(mbft_ctx* ctx, uint32_t role, const uint8_t* msg,
                                     size_t msg_len, uint8_t* tag_out, size_t tag_cap,
                                     size_t* tag_len);

/* crypto/ecdsa.Verify core over decoded items.  e, r, s: n x 32 bytes
 * big-endian (e = hashToInt input, i.e. the left-most 32 bytes of the
 * digest, zero-padded on the LEFT if the digest is shorter); slots from
 * mbft_key_slot / mbft_register_points.  status: n bytes (mbft_status). */
int mbft_verify_prehashed(mbft_ctx* ctx, const uint8_t* e, const uint8_t* r, const uint8_t* s,
                          const uint32_t* slots, size_t n, uint8_t* status);
int mbft_verify_prehashed_device(mbft_ctx* ctx, const uint8_t* d_e, const uint8_t* d_r,
                                 const uint8_t* d_s, const uint32_t* d_slots, size_t n,
                                 uint8_t* d_status, void* hip_stream);

/* The inline-key class: verify under keys GIVEN WITH THE CALL, no slot, no
 * registration (the coldest rung of the key ladder: zero bytes, zero state).
 * This is the reference's own boundary -- crypto/ecdsa.Verify(pub, hash, r, s)
 * at sample/authentication/crypto.go:86 and usig/sgx/usig-enclave.go:224, and
 * AuthenticationScheme.VerifyAuthenticationTag(m, sig, pubKey) at
 * crypto.go:95-98 and 120-126 take the key per call.
 *
 * mbft_verify_prehashed_keys / _device: xy is n x 64 bytes, big-endian
 * X || Y, as mbft_register_points takes them; e, r, s as above.  status[i] is
 * exactly what mbft_verify_prehashed returns for (e, r, s)[i] under a slot that
 * mbft_register_points gave xy[i]: MBFT_ACCEPT or MBFT_REJECT_SIG for a valid
 * point; MBFT_BAD_KEY for X >= p, Y >= p or a point off the curve ((0, 0)
 * among them), also where r or s is out of range; MBFT_REJECT_SIG for a valid
 * point with r or s outside [1, N).  Each point is validated on the GPU, then
 * used by the table-free keys' ladder: every degenerate case is exact.
 *
 * mbft_scheme_verify_flat32: PublicAuthenScheme.VerifyAuthenticationTag(m, sig,
 * pk) of the ECDSA roles (crypto.go:120-126 -> 79-89), n calls: call i =
 * (msgs[msg_off[i] .. msg_off[i+1]), tags[tag_off[i] .. tag_off[i+1]),
 * xy[64 i ..]).  e = (m || SHA256(""))[0:32] (crypto.go:121; messages shorter
 * than 32 bytes and empty ones included); the tag by mbft_der_parse_sig's
 * rules: a parse error is MBFT_MALFORMED_DER (where Go panics) and wins over
 * MBFT_BAD_KEY, bytes after the SEQUENCE are ignored, an r or s outside
 * (0, 2^256) goes to the verifier as zero and is rejected there.  The host
 * decodes; only the undecided calls go to the GPU.  There is no USIG form
 * (that scheme keeps epoch state per key fingerprint).
 *
 * n == 0 returns MBFT_OK; a NULL buffer with n > 0 is MBFT_ERR_ARG.  The calls
 * read the context's generator table and nothing else: they work on a context
 * with no key at all, under any key class and generator window, and leave
 * slots, key memory, use counts and the verified-call memo untouched.  They
 * serialise on the context like mbft_verify_prehashed* and run on its own
 * device.  The _device form is asynchronous on hip_stream (NULL: the
 * context's).  Device pointers d_e, d_r, d_s and d_xy must be 16-byte aligned
 * (the kernels read them as 128-bit words) -- what the mbft_verify_prehashed_device
 * form requires of d_e, d_r, d_s as well. */
int mbft_verify_prehashed_keys(mbft_ctx* ctx, const uint8_t* e, const uint8_t* r, const uint8_t* s,
                               const uint8_t* xy, size_t n, uint8_t* status);
int mbft_verify_prehashed_keys_device(mbft_ctx* ctx, const uint8_t* d_e, const uint8_t* d_r,
                                      const uint8_t* d_s, const uint8_t* d_xy, size_t n,
                                      uint8_t* d_status, void* hip_stream);
int mbft_scheme_verify_flat32(mbft_ctx* ctx, const uint8_t* msgs, const uint32_t* msg_off,
                              const uint8_t* tags, const uint32_t* tag_off, const uint8_t* xy,
                              size_t n, uint8_t* status_out);

/* The P-384 class: the same boundary over secp384r1.  The reference's ECDSA
 * roles are not tied to one curve -- ecdsaKeySpec.generateKeyPair
 * (sample/authentication/keymanager.go:368-382) makes P-384 keys at security
 * parameter 384, parsePublicKey (:352-366, x509.ParsePKIXPublicKey) accepts
 * them and EcdsaSigCipher.Verify (crypto.go:79-89) calls the curve-generic
 * ecdsa.Verify.  Keys are given with the call, as in the inline-key class;
 * P-384 keys cannot be registered (mbft_set_public_key_pkix refuses them).
 *
 * mbft_verify_prehashed_p384_keys / _device: e, r, s are n x 48 bytes
 * big-endian (e = hashToInt(hash) for a 384-bit order: the left-most 48 bytes
 * of the digest, a shorter digest right-aligned; any value below 2^384, e >= N
 * included), xy is n x 96 bytes X || Y.  Statuses and their precedence are the
 * inline-key class's: MBFT_BAD_KEY for X >= p, Y >= p or a point off the curve
 * ((0, 0) among them), also where r or s is out of range; MBFT_REJECT_SIG for
 * a valid point with r or s outside [1, N), for a sum at infinity or an x
 * mismatch; else MBFT_ACCEPT.  One kernel, k_verify_p384: the lane validates
 * its key, inverts s and runs complete addition formulas -- every degenerate
 * case (Q = +-G, u1 G = +-u2 Q, u1 = 0) is exact.
 *
 * mbft_scheme_verify_p384_flat32: VerifyAuthenticationTag(m, sig, pk) of the
 * ECDSA roles (crypto.go:120-126 -> 79-89) as mbft_scheme_verify_flat32, xy
 * 96 bytes a call.  md = m || SHA256("") (crypto.go:121), L = len(m) + 32
 * bytes: e = md[0:48] for L >= 48; for messages under 16 bytes e is the whole
 * of md as a big-endian integer, right-aligned in 48 bytes (hashToInt does not
 * shift: the order's bit length is a byte multiple).  The tag by
 * mbft_der_parse_sig48's rules: a parse error is MBFT_MALFORMED_DER and wins
 * over MBFT_BAD_KEY, bytes after the SEQUENCE are ignored.
 *
 * mbft_der_parse_sig48: mbft_der_parse_sig at width 48 -- the same grammar,
 * the same `consumed`; a value outside (0, 2^384) goes on as zero.
 *
 * mbft_pkix_parse_p384: parsePublicKey for a P-384 key.  Accepts exactly the
 * 120-byte SubjectPublicKeyInfo of an uncompressed point (30 76 30 10 06 07 2a
 * 86 48 ce 3d 02 01 06 05 2b 81 04 00 22 03 62 00 04 || X || Y), validates the
 * point on the host as x509.ParsePKIXPublicKey does and writes X || Y to xy96.
 * MBFT_OK, or MBFT_ERR_KEY with mbft_set_public_key_pkix's messages on ctx
 * (ctx may be NULL: no message is kept).  Takes no lock, touches no GPU.
 *
 * Argument rules, locking and statelessness are the inline-key class's: n == 0
 * returns MBFT_OK, a NULL buffer with n > 0 is MBFT_ERR_ARG; the calls
 * serialise on the context, work on one with no key and no generator table,
 * and leave slots, key memory, use counts and the verified-call memo as they
 * were.  The _device form is asynchronous on hip_stream (NULL: the
 * context's); d_e, d_r, d_s and d_xy must be 16-byte aligned. */
int mbft_verify_prehashed_p384_keys(mbft_ctx* ctx, const uint8_t* e, const uint8_t* r, const uint8_t* s,
                                    const uint8_t* xy, size_t n, uint8_t* status);
int mbft_verify_prehashed_p384_keys_device(mbft_ctx* ctx, const uint8_t* d_e, const uint8_t* d_r,
                                           const uint8_t* d_s, const uint8_t* d_xy, size_t n,
                                           uint8_t* d_status, void* hip_stream);
int mbft_scheme_verify_p384_flat32(mbft_ctx* ctx, const uint8_t* msgs, const uint32_t* msg_off,
                                   const uint8_t* tags, const uint32_t* tag_off, const uint8_t* xy,
                                   size_t n, uint8_t* status_out);
int mbft_der_parse_sig48(const uint8_t* sig, size_t len, uint8_t r48[48], uint8_t s48[48],
                         size_t* consumed);
int mbft_pkix_parse_p384(mbft_ctx* ctx, const uint8_t* pkix, size_t len, uint8_t xy96[96]);

/* Bulk ECDSA signing over decoded digests, for synthetic load generation
 * and tests (the signature format of crypto.go:63-76).  priv32: nkeys x 32 B
 * big-endian scalars; key_idx: n indices (NULL = key 0); e: n x 32 B; r, s:
 * n x 32 B big-endian outputs.  Deterministic nonce.  NOT CONSTANT-TIME:
 * its memory accesses depend on the nonce; never give it a key that
 * protects anything. */
int mbft_sign_prehashed(mbft_ctx* ctx, const uint8_t* priv32, size_t nkeys,
                        const uint32_t* key_idx, const uint8_t* e, size_t n, uint8_t* r_out,
                        uint8_t* s_out);
int mbft_sign_prehashed_device(mbft_ctx* ctx, const uint8_t* d_priv32, const uint32_t* d_key_idx,
                               const uint8_t* d_e, size_t n, uint8_t* d_r, uint8_t* d_s,
                               void* hip_stream);

/* Signing with GIVEN nonces k (n x 32 B big-endian, 1 <= k < N): r = x(kG)
 * mod N, s = k^-1 (e + r d) mod N; a bad nonce gives r = s = 0.  For
 * constructing crafted inputs (bench.py's adversarial lines: items whose u2
 * has a zero comb window), never used for real tags. */
int mbft_sign_nonce_device(mbft_ctx* ctx, const uint8_t* d_priv32, const uint32_t* d_key_idx,
                           const uint8_t* d_e, const uint8_t* d_k, size_t n, uint8_t* d_r,
                           uint8_t* d_s, void* hip_stream);

/* SHA-256 stage on the GPU over device buffers, on the caller's stream
 * (north_star item 3: AuthenBytes construction feeds a GPU SHA-256 stage).
 *   mbft_request_digests_device: the ECDSA-role digest input of n REQUESTs,
 *     e_i = (AuthenBytes(REQUEST_i) || SHA256(""))[0:32]
 *         = "REQUEST" || seq_be64 || SHA256(op_i)[0:17]
 *     (messages/authen.go:33,54-56 + sample/authentication/crypto.go:121);
 *     ops: n x op_len bytes back to back; seq: n u64.
 *   mbft_sha256_device: out_i = SHA256(data[off_i, off_{i+1})), the hashsum
 *     of messages/authen.go:78-82; off: n + 1 byte offsets.
 *   mbft_usig_digests_device: e_i = SHA256(SHA256(m_i) || epoch_le64 ||
 *     counter_le64), the USIG signed digest (usig/sgx/sgx-usig.go:99-101,
 *     usig/sgx/usig-enclave.go:204-214); m_i = data[off_i, off_{i+1}).
 * Outputs are n x 32 bytes (big-endian digest bytes). */
int mbft_request_digests_device(mbft_ctx* ctx, const uint64_t* d_seq, const uint8_t* d_ops,
                                uint32_t op_len, size_t n, uint8_t* d_e, void* hip_stream);
int mbft_sha256_device(mbft_ctx* ctx, const uint8_t* d_data, const uint64_t* d_off, size_t n,
                       uint8_t* d_out, void* hip_stream);
int mbft_usig_digests_device(mbft_ctx* ctx, const uint8_t* d_data, const uint64_t* d_off,
                             const uint64_t* d_epoch, const uint64_t* d_counter, size_t n,
                             uint8_t* d_e, void* hip_stream);

/* Kernel timing: when enabled, HIP events bracket the batched-inversion and
 * verify kernels of every verify call, on the stream they run on.
 * mbft_profile_read fills out[0] = total verify-kernel ms, out[1] = total
 * inversion ms, out[2] = batches, out[3] = items, and resets the totals. */
int mbft_profile_enable(mbft_ctx* ctx, int enable);
int mbft_profile_read(mbft_ctx* ctx, double out[4]);
/* Host-side stage times of mbft_verify_batch since the last read (always
 * collected): out[0] = batches, out[1] = items, out[2] = host per-call work
 * (role/key lookup, DER decode, digest construction, staging writes; ms,
 * overlapped with the previous chunk's transfers and kernels), out[3] = wait
 * for the GPU after the last chunk was enqueued (ms), out[4] = in-order
 * resolution incl. the USIG epoch replay (ms), out[5] = wall total (ms).
 * Resets the totals. */
int mbft_profile_stages(mbft_ctx* ctx, double out[6]);
/* The device message layer (mbft_validate_messages_flat,
 * mbft_check_messages_flat) while profiling is enabled, from HIP events:
 * out[0] = calls, out[1] = H2D ms (the records' and arena's uploads on the
 * copy stream, first copy start to last copy end), out[2] = device ms (first
 * copy start to the end of the last kernel / download), out[3] = bytes
 * uploaded; summed over the context and its lanes, then reset. */
int mbft_profile_msg_layer(mbft_ctx* ctx, double out[4]);

/* ---------------------------------------------------------------------------
 * MinBFT message layer.
 *
 * mbft_message flattens a message's authenticated fields
 * (messages/authen.go:52-76, messages/api.go):
 *   REQUEST          client_id, seq, op, sig
 *   REPLY            replica_id, client_id, seq, op (= result), sig
 *                    (client side only: mbft_validate_replies)
 *   PREPARE          replica_id (primary), view, client_id, seq, op, sig (of
 *                    the embedded REQUEST), ui_counter/ui_cert
 *   COMMIT           replica_id, prep_replica_id, view, client_id, seq, op,
 *                    sig, prep_ui_counter/prep_ui_cert (the embedded
 *                    PREPARE's UI), ui_counter/ui_cert
 *   REQ-VIEW-CHANGE  view (= the new view)
 * `stream` identifies the peer/client stream the message arrived on. */
enum mbft_msg_type {
  MBFT_MSG_REQUEST = 1,
  MBFT_MSG_REPLY = 2,
  MBFT_MSG_PREPARE = 3,
  MBFT_MSG_COMMIT = 4,
  MBFT_MSG_REQ_VIEW_CHANGE = 5
};

typedef struct mbft_message {
  uint32_t type;
  uint32_t stream;
  uint32_t replica_id;
  uint32_t prep_replica_id;
  uint64_t view;
  uint32_t client_id;
  uint32_t reserved;
  uint64_t seq;
  const uint8_t* op;
  size_t op_len;
  const uint8_t* sig;
  size_t sig_len;
  uint64_t ui_counter;
  const uint8_t* ui_cert;
  size_t ui_cert_len;
  uint64_t prep_ui_counter;
  const uint8_t* prep_ui_cert;
  size_t prep_ui_cert_len;
} mbft_message;

/* Validation result per message: 0 = valid, else (stage << 8) | mbft_status
 * of the failing check (status 0 for checks that are not authenticator
 * calls). */
enum mbft_stage {
  MBFT_ST_REQUEST_SIG = 1,         /* core/request.go:146-150 (also inside PREPARE/COMMIT) */
  MBFT_ST_NOT_PRIMARY = 2,         /* core/prepare.go:51-53 "Prepare from backup" */
  MBFT_ST_PREPARE_UI = 3,          /* core/prepare.go:59-61 + core/usig-ui.go:62-77 */
  MBFT_ST_COMMIT_FROM_PRIMARY = 4, /* core/commit.go:78-80 */
  MBFT_ST_COMMIT_UI = 5,           /* core/commit.go:86-88 */
  MBFT_ST_NOT_IMPLEMENTED = 6,     /* core/message-handling.go:418-419 (ReqViewChange) */
  MBFT_ST_STREAM_STOPPED = 7,      /* an earlier message of the stream was rejected
                                      (core/message-handling.go:217-220) */
  MBFT_ST_REPLY_SIG = 8,           /* client/message-handling.go:161-170 */
  MBFT_ST_AFTER_PANIC = 9,         /* an earlier message made Go panic (crypto.go:82-84) */
  MBFT_ST_UNKNOWN_TYPE = 10,       /* a REPLY in a replica's stream: the message
                                      validator panics (core/message-handling.go:420-421) */
  MBFT_ST_REPLY_CLIENT_ID = 11     /* client/message-handling.go:163-165 "Client ID mismatch" */
};

enum mbft_validate_flags { MBFT_VF_NO_STREAM_STOP = 1, MBFT_VF_NO_PANIC_STOP = 2 };

/* messages.AuthenBytes (messages/authen.go:27-50): writes into out (cap
 * bytes), *len = required size (MBFT_ERR_ARG if cap is too small). */
int mbft_authen_bytes(const mbft_message* m, uint8_t* out, size_t cap, size_t* len);

/* The digest input e of the authenticator call over AuthenBytes(msgs[i]),
 * built on the GPU from the raw fields (SHA256(op) by k_sha256_var, the
 * AuthenBytes layout of messages/authen.go:52-76 in registers by
 * k_authen_e), one host round trip:
 *   kind 0  REQUEST, ECDSA role:  e = (AuthenBytes || SHA256(""))[0:32]
 *   kind 1  REPLY, ECDSA role:    the same over the REPLY layout
 *   kind 2  PREPARE, USIG:  e = SHA256(SHA256(AuthenBytes) || epochs[i]_le || counters[i]_le)
 *   kind 3  COMMIT, USIG:   the same over the COMMIT layout (prep_replica_id,
 *                           prep_ui_counter)
 * (crypto.go:121; sgx-usig.go:99-101, usig-enclave.go:204-214).  e_out: n x
 * 32 bytes.  mbft_validate_messages / _replies use the same stage. */
int mbft_authen_digests(mbft_ctx* ctx, const mbft_message* msgs, size_t n, uint32_t kind,
                        const uint64_t* epochs, const uint64_t* counters, uint8_t* e_out);

/* Validates n messages in order exactly as the core's messageValidator would,
 * one stream loop per `stream` value, with all signature checks of the batch
 * on the GPU (identical authenticator calls verified once).  n_replicas is
 * the `n` of isPrimary (view mod n).  out: n results as above. */
int mbft_validate_messages(mbft_ctx* ctx, const mbft_message* msgs, size_t n, uint32_t n_replicas,
                           uint32_t flags, int32_t* out);

/* The same validation over a FLAT batch (new; replaces the same
 * core/message-handling.go:409-424 validator loop as mbft_validate_messages):
 * one fixed-size record per message with the variable-length fields as
 * offsets into one byte arena -- no pointers, so Go can marshal a batch
 * straight into C memory.  When `recs` and `bytes` lie in library page-locked
 * memory (mbft_host_alloc), the whole message layer runs on the GPU: the
 * records and bytes go up raw, and the candidate calls of every message, their
 * content hashes and the deduplication (a device hash table, first occurrence
 * in message order wins, every hash hit compared in full), the AuthenBytes +
 * SHA-256 digests, Go-exact DER, the USIG UI / cert split and the key lookups
 * are all kernels (msg_kernels.hip); the host only replays the results in
 * message order (stream stop, panic stop, USIG epoch state).  Otherwise (or
 * past 2^28 messages in one call) the records are turned into mbft_message
 * structs over `bytes` and validated by mbft_validate_messages.  Results are identical either way.  Offsets are
 * byte offsets into `bytes` (nbytes long); a field of length 0 may carry any
 * offset.  mbft_pack_messages builds such a batch from mbft_message structs
 * (the bytes each message points to, copied): *used = the arena bytes the
 * batch needs (recs == NULL: only that), MBFT_ERR_ARG when cap is too small. */
typedef struct mbft_msg_rec {
  uint32_t type;
  uint32_t stream;
  uint32_t replica_id;
  uint32_t prep_replica_id;
  uint32_t client_id;
  uint32_t op_len;
  uint32_t sig_len;
  uint32_t ui_cert_len;
  uint32_t prep_ui_cert_len;
  uint32_t reserved;
  uint64_t view;
  uint64_t seq;
  uint64_t ui_counter;
  uint64_t prep_ui_counter;
  uint64_t op_off;
  uint64_t sig_off;
  uint64_t ui_cert_off;
  uint64_t prep_ui_cert_off;
} mbft_msg_rec;

int mbft_validate_messages_flat(mbft_ctx* ctx, const mbft_msg_rec* recs, size_t n,
                                const uint8_t* bytes, size_t nbytes, uint32_t n_replicas,
                                uint32_t flags, int32_t* out);
int mbft_pack_messages(const mbft_message* msgs, size_t n, mbft_msg_rec* recs, uint8_t* bytes,
                       size_t cap, size_t* used);

/* The same validation split in two, like mbft_check_batch /
 * mbft_resolve_checked (new; for the core's stream loop,
 * core/message-handling.go:204-246, which validates each message right
 * before processing it and ends the stream at the first error):
 *   mbft_check_messages_flat  every signature, digest, DER / UI decode and key
 *                      lookup of the batch on the GPU at once (the device
 *                      message layer above), NO state read or written; the
 *                      per-message checks are kept in *out;
 *   mbft_resolve_message  later, per message, in the caller's order: message
 *                      i's result (0, or (stage << 8) | status, as above),
 *                      applying the USIG epoch step (crypto.go:219-236) to
 *                      the context's state at that moment -- no GPU work.
 * No stream stop and no panic stop: each message's own result (the caller's
 * loop stops itself; MBFT_MALFORMED_DER at MBFT_ST_REQUEST_SIG /
 * MBFT_ST_REPLY_SIG and MBFT_ST_UNKNOWN_TYPE are where Go panics).
 * Resolving messages 0 .. n-1 in order gives what mbft_validate_messages_flat
 * gives with MBFT_VF_NO_STREAM_STOP | MBFT_VF_NO_PANIC_STOP; a message never
 * resolved leaves the epoch state untouched, as a message the reference never
 * validates.  recs / bytes outside library page-locked memory are staged into
 * the engine's own first.  Runs on a concurrency lane (mbft_set_concurrency)
 * when there are several; resolve takes the context lock briefly.
 * mbft_msg_batch_free releases the batch (any time after the check). */
typedef struct mbft_msg_batch mbft_msg_batch;
int mbft_check_messages_flat(mbft_ctx* ctx, const mbft_msg_rec* recs, size_t n, const uint8_t* bytes,
                             size_t nbytes, uint32_t n_replicas, mbft_msg_batch** out);
int mbft_resolve_message(mbft_ctx* ctx, mbft_msg_batch* batch, size_t i);
/* count consecutive messages i0 .. i0+count-1 resolved in order into out[]:
 * the same as count mbft_resolve_message calls, one lock and one call. */
int mbft_resolve_messages(mbft_ctx* ctx, mbft_msg_batch* batch, size_t i0, size_t count,
                          int32_t* out);
void mbft_msg_batch_free(mbft_msg_batch* batch);
/* Coalescing of concurrent mbft_check_messages_flat calls (new; the core
 * runs one stream loop per peer connection, core/message-handling.go:
 * 250-275, so a replica's streams check their batches at the same time).
 * When enabled, a call that arrives while another pass holds the engine
 * queues; the first queued caller leads the next pass, which takes every
 * queued batch with the same n_replicas (up to max_messages messages; 0:
 * 2^20) and checks them as ONE device pass -- records and arenas
 * concatenated into the library's page-locked staging, identical calls
 * across the batches verified once -- and every caller gets its own
 * mbft_msg_batch (results exactly as if checked alone: a check touches no
 * state; the USIG epoch step stays in each caller's resolve).  A caller
 * whose records would fail alone (unknown type, field outside its arena)
 * gets MBFT_ERR_ARG and the others are unaffected.  max_wait_us > 0 lets a
 * leader wait that long for company first.  Default: disabled.
 * mbft_check_coalescing_stats: out[0] passes, out[1] caller batches,
 * out[2] messages since the last call (then reset). */
int mbft_set_check_coalescing(mbft_ctx* ctx, int enabled, uint32_t max_wait_us, size_t max_messages);
int mbft_check_coalescing_stats(mbft_ctx* ctx, double out[3]);
/* Small checks (new): a check pass of at most max_messages messages (one
 * caller's batch, or a coalesced pass; default 512, 0 = never) skips the
 * device message layer's fixed cost -- record upload, dedup table, scan,
 * several launches, two host waits -- for the latency of the core's
 * one-message-at-a-time streams (a client's REQUEST stream is strictly
 * sequential, core/message-handling.go:399): the checks and candidate calls
 * are built and deduplicated on the host (content hash, full compares), the
 * AuthenBytes digests hashed on the host (SHA extensions), and the unique
 * calls verified in ONE launch of the small-batch kernel (from zero-copy
 * staging up to 256 calls, s^-1 inverted on the host up to 64) -- the
 * lone-call path.  1 message: ~36 us against ~270 us through the device
 * layer (15-23 us through the resident verifier); 256 messages ~165 us
 * against ~430 us, 512 messages ~315 us against ~440-500 us, 1024 ~500 us
 * against ~450-480 us (tools/lowload_probe.py), hence 512.  Identical
 * results; records
 * and arena may lie in any host memory. */
int mbft_set_small_check(mbft_ctx* ctx, size_t max_messages);

/* Client side: validates n REPLY messages as the client `client_id` does
 * (client/message-handling.go:93-110,140-170): ClientID mismatch ->
 * MBFT_ST_REPLY_CLIENT_ID, else VerifyMessageAuthenTag(ReplicaAuthen,
 * replica_id, AuthenBytes(REPLY), sig) -> 0 or (MBFT_ST_REPLY_SIG << 8 |
 * status).  A rejected REPLY does not stop its stream (the client only logs
 * it); a malformed DER signature panics (then MBFT_ST_AFTER_PANIC, unless
 * MBFT_VF_NO_PANIC_STOP).  Non-REPLY messages -> MBFT_ERR_ARG. */
int mbft_validate_replies(mbft_ctx* ctx, const mbft_message* msgs, size_t n, uint32_t client_id,
                          uint32_t flags, int32_t* out);
/* The same over a flat batch (records + one byte arena, as
 * mbft_validate_messages_flat; new): what the Go client's batched reply loop
 * marshals (go/gpuauth/replies.go).  Batches of up to mbft_set_small_check's
 * size take the small route (AuthenBytes hashed on the host, one zero-copy
 * verify launch), larger ones the GPU digest stage. */
int mbft_validate_replies_flat(mbft_ctx* ctx, const mbft_msg_rec* recs, size_t n, const uint8_t* bytes,
                               size_t nbytes, uint32_t client_id, uint32_t flags, int32_t* out);

/* Batch GenerateMessageAuthenTag for the ECDSA roles (new): n calls of
 * api.Authenticator.GenerateMessageAuthenTag (api/api.go:133-144) -> the
 * ecdsaSigCipher.Sign of sample/authentication/crypto.go:57-76 at once, with
 * the role's private key from mbft_set_private_key, fit for real keys: the
 * kernel's memory addresses, branches and loop counts do not depend on the
 * key or the nonce.  The nonce is RFC 6979 (HMAC-SHA-256)
 * where the reference draws from crypto/rand (crypto.go:65): tags are
 * reproducible, verification does not depend on it.  Each tag is
 * asn1.Marshal(ecdsaSignature{R, S}) (crypto.go:69) in a slot of
 * MBFT_TAG_SLOT bytes (the rest of the slot zeroed), its length in
 * tag_len[i]; an item that found no nonce in 4 candidates (unreachable in
 * practice) gets length 0.  role: MBFT_ROLE_REPLICA or MBFT_ROLE_CLIENT; a
 * role without a private key, or MBFT_ROLE_USIG (UIs come from
 * mbft_usig_create_uis_*), -> MBFT_ERR_STATE.  mbft_clear_keys also drops the private keys of these entry
 * points (device copies zeroed, then freed): MBFT_ERR_STATE until
 * mbft_set_private_key is called again.  Host buffers may be any memory.
 *   mbft_generate_tags_prehashed  e: n x 32 bytes, the hashToInt input
 *     (crypto.go:114,121 -> crypto/ecdsa.Sign).
 *   mbft_generate_tags_flat  raw AuthenBytes msgs[msg_off[i], msg_off[i+1]):
 *     e_i = (m_i || SHA256(""))[0:32] (crypto.go:114,121), built on the GPU.
 *   mbft_generate_tags_prehashed_device  device buffers (d_e 4-byte aligned),
 *     on the caller's stream, no synchronisation; the caller finishes that
 *     stream's work before it changes keys.
 *   mbft_sign_messages_flat  what the core and the client sign, from records
 *     and arena as mbft_validate_messages_flat takes them: REPLY
 *     (core/utils.go:43-53, core/message-handling.go:552-568) and
 *     REQ-VIEW-CHANGE with the replica key, REQUEST (client/request.go:
 *     194-204) with the client key; AuthenBytes (messages/authen.go:27-82,
 *     SHA256 of op / result included) and e are built on the GPU in the same
 *     kernel.  PREPARE / COMMIT (they carry a USIG UI, not an ECDSA-role tag:
 *     mbft_usig_sign_messages_flat below) or an unknown type, or an op outside
 *     the arena -> MBFT_ERR_ARG, nothing written.
 *   mbft_set_signer_window  the signer's generator table: 4, 5 (default) or
 *     6 bits per window (33 / 52 / 87 KB, 64 / 52 / 43 additions); the table
 *     is rebuilt on the next call, which first waits for the whole device
 *     (a _device call on the caller's stream may still read the old one). */
#define MBFT_TAG_SLOT 72
int mbft_generate_tags_prehashed(mbft_ctx* ctx, uint32_t role, const uint8_t* e, size_t n,
                                 uint8_t* tags, uint8_t* tag_len);
int mbft_generate_tags_flat(mbft_ctx* ctx, uint32_t role, const uint8_t* msgs,
                            const uint32_t* msg_off, size_t n, uint8_t* tags, uint8_t* tag_len);
int mbft_generate_tags_prehashed_device(mbft_ctx* ctx, uint32_t role, const uint8_t* d_e, size_t n,
                                        uint8_t* d_tags, uint8_t* d_tag_len, void* hip_stream);
int mbft_sign_messages_flat(mbft_ctx* ctx, const mbft_msg_rec* recs, size_t n, const uint8_t* bytes,
                            size_t nbytes, uint8_t* tags, uint8_t* tag_len);
int mbft_set_signer_window(mbft_ctx* ctx, int wbits);

/* A software USIG (new): CreateUI for PREPARE and COMMIT on hosts without SGX
 * (an MI355X host is an EPYC machine).  Replaces the enclave's
 * ecall_usig_create_ui (usig/sgx/enclave/usig.c:36-76) with its Go wrapper
 * (usig/sgx/sgx-usig.go:52-64 CreateUI, :71-79 ID), batch by batch, through
 * the uniform-access signer of the entry points above (k_usig_uis; RFC 6979
 * nonce, so a UI is reproducible from (d, epoch, counter, message)).
 *
 * NO TRUSTED HARDWARE.  MinBFT tolerates f < n/2 faults only because a faulty
 * replica cannot make its USIG sign two messages under one counter.  Here the
 * counter and the key are ordinary process state: whoever controls the host
 * controls them.  This is the equivalent of the SGX SDK's simulation mode --
 * for development, tests and benchmarks on this machine class -- and the Go
 * binding keeps it off unless asked (Config.GPUUSIG).
 *
 * Semantics kept from the enclave: the epoch is fixed per instance; the
 * counter starts at 1 and moves only when valid signatures are handed out;
 * the signed digest is SHA256(SHA256(m) || epoch_le64 || counter_le64)
 * (sgx-usig.go:99-101, usig-enclave.go:204-214); a UI is counter_be64 ||
 * epoch_be64 || asn1.Marshal{R, S} (usig/usig.go:54-86, sgx-usig.go:143-168),
 * at most MBFT_UI_SLOT bytes: each UI sits in a slot of that size, the rest
 * of the slot zeroed, its length in ui_len[i].
 *
 * The counter contract: calls on one context are serialised; a call takes the
 * counters [next, next + n) for items 0 .. n-1, runs the kernel, copies the
 * UIs out and only then advances next by n, reporting the first counter in
 * *first_counter.  If anything fails (launch, copy, an item without a usable
 * nonce) the call returns an error, zeroes uis and ui_len, and leaves the
 * counter where it was: no counter value appears in two UIs that left the
 * library, and successful calls leave no gaps (peerstate's CaptureUI waits
 * forever on a gap).  There is no device-pointer / caller-stream form: without
 * a synchronisation the library could not know that a UI was exposed.  The
 * counter is not persisted: a restart is a new instance with a new epoch, as
 * for the enclave.  On a multi-device context the instance lives on the
 * context's first device.
 *   mbft_usig_init  a new instance: key d (32 B big-endian, into a device
 *     buffer that is zeroed before it is freed), the epoch (the enclave draws
 *     it from sgx_read_rand, usig.c:177-184: pass random bits), counter 1.
 *     d = 0 or d >= N -> MBFT_ERR_KEY; an epoch equal to that of this
 *     context's previous instance -> MBFT_ERR_STATE (either leaves an existing
 *     instance as it is).  Replaces an existing instance.  Independent of
 *     mbft_set_private_key(MBFT_ROLE_USIG, ...), which it neither reads nor
 *     changes.  mbft_clear_keys and mbft_ctx_destroy drop the instance (key
 *     zeroed, then freed): every entry point here is MBFT_ERR_STATE until the
 *     next mbft_usig_init, which needs a fresh epoch.
 *   mbft_usig_id  the identity epoch_be64 || PKIX(d G) (sgx-usig.go:105-139),
 *     MBFT_USIG_ID_LEN bytes; *len receives that size, MBFT_ERR_ARG when cap
 *     is smaller.  d G comes from the same uniform comb as a nonce's point.
 *   mbft_usig_next_counter  the counter the next UI will carry.
 *   mbft_usig_create_uis_digests  UI i over the message whose SHA256 is
 *     digests[32 i .. 32 i + 32).
 *   mbft_usig_create_uis_flat  UI i over the raw message
 *     msgs[msg_off[i], msg_off[i+1]), hashed on the GPU.
 *   mbft_usig_sign_messages_flat  UI i over AuthenBytes(recs[i])
 *     (messages/authen.go:27-82) for PREPARE (core/prepare.go) and COMMIT
 *     (core/commit.go: prep_replica_id and prep_ui_counter name the PREPARE)
 *     records over an arena, as mbft_validate_messages_flat takes them, built
 *     and hashed on the GPU.  Any other type, or an op outside the arena ->
 *     MBFT_ERR_ARG, nothing written, the counter untouched. */
#define MBFT_UI_SLOT 88
#define MBFT_USIG_ID_LEN 99
int mbft_usig_init(mbft_ctx* ctx, const uint8_t d[32], uint64_t epoch);
int mbft_usig_id(mbft_ctx* ctx, uint8_t* out, size_t cap, size_t* len);
int mbft_usig_next_counter(mbft_ctx* ctx, uint64_t* counter);
int mbft_usig_create_uis_digests(mbft_ctx* ctx, const uint8_t* digests, size_t n, uint8_t* uis,
                                 uint8_t* ui_len, uint64_t* first_counter);
int mbft_usig_create_uis_flat(mbft_ctx* ctx, const uint8_t* msgs, const uint32_t* msg_off, size_t n,
                              uint8_t* uis, uint8_t* ui_len, uint64_t* first_counter);
int mbft_usig_sign_messages_flat(mbft_ctx* ctx, const mbft_msg_rec* recs, size_t n, const uint8_t* bytes,
                                 size_t nbytes, uint8_t* uis, uint8_t* ui_len, uint64_t* first_counter);

/* Host-only helpers (no GPU). */
/* encoding/asn1 DER decode of struct{R, S *big.Int}.
 * Returns 1 on success, 0 on a Go asn1 error.  On success: *consumed = bytes
 * of the outer SEQUENCE (the rest is Go's `rest`); r32/s32 receive the value
 * if 0 < value < 2^256, else zero (Go: r <= 0 or r >= N -> Verify false). */
int mbft_der_parse_sig(const uint8_t* sig, size_t len, uint8_t r32[32], uint8_t s32[32],
                       size_t* consumed);
void mbft_sha256(const uint8_t* data, size_t len, uint8_t out[32]);
/* mbft_sha256 through one host compression (test hook): form 0 the portable
 * one, form 1 the x86 SHA extensions (MBFT_ERR_STATE when the CPU lacks
 * them).  mbft_sha256 and every host digest use form 1 where available. */
int mbft_debug_sha256(int form, const uint8_t* data, size_t len, uint8_t out[32]);

#ifdef __cplusplus
}
#endif

#endif /* MINBFT_GPU_H */
