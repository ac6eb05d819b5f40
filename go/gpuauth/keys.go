package gpuauth

// Which keys the GPU context holds.  The reference's authenticator verifies
// a call by ANY id its key store has a key for (SimpleKeyStore.NodePublicKey,
// sample/authentication/keymanager.go:96-101, over every key of keys.yaml,
// :179-227), so the binding must too:
//
//   - KeyIDsFromFile lists every id of every role in a keys.yaml (the file
//     LoadSimpleKeyStore reads), so a replica registers all of them at start
//     (sample/peer/cmd/gpu-stack.go), whatever their number or numbering;
//   - with Config.KeyStore set, a call whose (role, id) the context does not
//     hold yet is looked up in the store BEFORE its batch goes to the GPU
//     (ensureKeys) and, if the store has the key, registered first, at the
//     comb window of its role.  Registering before the batch -- not retrying
//     after an MBFT_UNKNOWN_KEY -- keeps every status, and the USIG epoch
//     state, exactly what the reference gives: the batch runs as if the key
//     had been there from the start.  An id the store does not have is
//     remembered as absent (the store is static) and rejected as the
//     reference rejects it (a nil key, crypto.go:85-88 / :192-195);
//   - RemoveKey, SetKeyClass, KeyUsage and PromoteHotKeys are the life of a
//     key after that (include/minbft_gpu.h): a client that left gives its
//     slot and table back, a hot key gets a table.  A removed key that the
//     store still has comes back through ensureKey on its next call;
//   - SetKeyBudget, RebalanceKeys, AgeKeyUsage and ColdKeys keep that life
//     within a memory budget (Config.KeyBudget runs them on a clock): cold
//     keys lose their tables and hot ones gain them, counts fade, and client
//     keys nobody uses are evicted.

/*
#include "minbft_gpu.h"
*/
import "C"

import (
	"crypto/ecdsa"
	"fmt"
	"io"
	"io/ioutil"
	"sort"
	"sync"
	"sync/atomic"
	"unsafe"

	yaml "gopkg.in/yaml.v2"

	"github.com/hyperledger-labs/minbft/api"
)

// keyFile is the part of the reference's key store file the binding reads:
// the ids of each role's key set (keymanager.go:147-171 simpleKeyStoreFile,
// keySet, keyPair; the keys themselves come from the loaded store).
type keyFile struct {
	Replica *keyFileSet `yaml:"replica"`
	Usig    *keyFileSet `yaml:"usig"`
	Client  *keyFileSet `yaml:"client"`
}

type keyFileSet struct {
	Keys []keyFileEntry `yaml:"keys"`
}

type keyFileEntry struct {
	ID uint32 `yaml:"id"`
}

// KeyIDsFromFile returns, per role, the sorted ids that have a key in a
// keys.yaml.  A role whose key set is present has an entry even with no
// keys (the reference then knows the role: an unknown id is "invalid
// signature", not "key set not found", keymanager.go:96-101).
func KeyIDsFromFile(r io.Reader) (map[api.AuthenticationRole][]uint32, error) {
	b, err := ioutil.ReadAll(r)
	if err != nil {
		return nil, fmt.Errorf("read error: %v", err)
	}
	var f keyFile
	if err := yaml.Unmarshal(b, &f); err != nil {
		return nil, fmt.Errorf("yaml parse error: %v", err)
	}
	out := make(map[api.AuthenticationRole][]uint32)
	for role, set := range map[api.AuthenticationRole]*keyFileSet{
		api.ReplicaAuthen: f.Replica, api.USIGAuthen: f.Usig, api.ClientAuthen: f.Client} {
		if set == nil {
			continue
		}
		ids := make([]uint32, 0, len(set.Keys))
		for _, k := range set.Keys {
			ids = append(ids, k.ID)
		}
		sort.Slice(ids, func(i, j int) bool { return ids[i] < ids[j] })
		out[role] = ids
	}
	return out, nil
}

type roleID struct {
	role api.AuthenticationRole
	id   uint32
}

// maxAbsent bounds the remembered absent ids (a peer may send any id).
const maxAbsent = 1 << 16

// keyRegistry tracks the (role, id) pairs the context holds and the ones the
// key store does not have, and registers late keys.
type keyRegistry struct {
	mu      sync.RWMutex
	ks      PublicKeyStore
	windows Windows
	known   map[roleID]bool
	absent  map[roleID]bool
}

func (r *keyRegistry) init(ks PublicKeyStore, w Windows) {
	r.ks = ks
	r.windows = w
	r.known = make(map[roleID]bool)
	r.absent = make(map[roleID]bool)
}

func (r *keyRegistry) add(role api.AuthenticationRole, id uint32) {
	r.mu.Lock()
	r.known[roleID{role, id}] = true
	r.mu.Unlock()
}

// ensure makes sure (role, id) is registered if the key store has a key for
// it.  Cheap when it is known or known absent (a read-locked map lookup).
func (a *Authenticator) ensureKey(role api.AuthenticationRole, id uint32) {
	r := &a.keys
	if r.ks == nil {
		return
	}
	if roleByte(role) == 0 {
		return // no scheme for the role: rejected as MBFT_UNKNOWN_ROLE whatever a key store holds
	}
	k := roleID{role, id}
	r.mu.RLock()
	done := r.known[k] || r.absent[k]
	r.mu.RUnlock()
	if done {
		return
	}
	r.mu.Lock()
	defer r.mu.Unlock()
	if r.known[k] || r.absent[k] {
		return
	}
	miss := func() {
		if len(r.absent) >= maxAbsent {
			r.absent = make(map[roleID]bool)
		}
		r.absent[k] = true
	}
	pk, err := r.ks.NodePublicKey(role, id)
	if err != nil || pk == nil {
		miss() // no key set for the role, or no key for the id: the reference rejects
		return
	}
	epk, ok := pk.(*ecdsa.PublicKey)
	if !ok {
		miss()
		return
	}
	xy, err := rawXY(epk)
	if err != nil {
		miss()
		return
	}
	// the context-wide "window for keys registered next": set under r.mu,
	// the only place keys are added after New
	if setKeyClass(a.ctx, r.windows, role) != C.MBFT_OK {
		return // left unknown: the call is rejected as with no key, retried next time
	}
	C.mbft_add_role(a.ctx, C.uint32_t(role))
	if C.mbft_set_public_key_xy(a.ctx, C.uint32_t(role), C.uint32_t(id),
		(*C.uint8_t)(unsafe.Pointer(&xy[0]))) != C.MBFT_OK {
		return
	}
	r.known[k] = true
}

// ensureKeys runs ensureKey over the signers of a batch (consecutive calls
// by the same signer are looked up once).
func (a *Authenticator) ensureKeys(calls []Call) {
	if a.keys.ks == nil {
		return
	}
	var last roleID
	for i, c := range calls {
		k := roleID{c.Role, c.ID}
		if i > 0 && k == last {
			continue
		}
		last = k
		a.ensureKey(c.Role, c.ID)
	}
}

// KeyClassTeeth is the class code of a compact key of t teeth
// (MBFT_KEY_CLASS_TEETH, a function-like macro cgo cannot call).
func KeyClassTeeth(t int) uint32 { return 0x100 | uint32(t) }

// KeyClassSignedTeeth is the class code of a signed compact key of t teeth
// (MBFT_KEY_CLASS_SIGNED_TEETH): 2^(t-1) entries of 64 bytes, t in 2..9.
func KeyClassSignedTeeth(t int) uint32 { return 0x200 | uint32(t) }

// RemoveKey unmaps (role, id) (mbft_remove_public_key): its calls are then
// rejected like those of an id never registered, and its slot and storage are
// reused once nothing else maps to them.  With Config.KeyStore set the key is
// registered again when a call by it arrives and the store still has it.
func (a *Authenticator) RemoveKey(role api.AuthenticationRole, id uint32) error {
	a.keys.mu.Lock()
	defer a.keys.mu.Unlock()
	rc := C.mbft_remove_public_key(a.ctx, C.uint32_t(roleByte(role)), C.uint32_t(id))
	if rc != C.MBFT_OK {
		return a.failure("mbft_remove_public_key", int(rc))
	}
	delete(a.keys.known, roleID{role, id})
	return nil
}

// SetKeyClass rebuilds the verification data of the registered key
// (role, id) in class cls: a comb window 4..29, MBFT_WINDOW_NONE or
// KeyClassTeeth(t) or KeyClassSignedTeeth(t).  On failure the key keeps its class.  One device
// synchronize a call.
func (a *Authenticator) SetKeyClass(role api.AuthenticationRole, id uint32, cls uint32) error {
	rc := C.mbft_set_key_class(a.ctx, C.uint32_t(roleByte(role)), C.uint32_t(id), C.uint32_t(cls))
	if rc != C.MBFT_OK {
		return a.failure("mbft_set_key_class", int(rc))
	}
	return nil
}

// KeyUsage returns the verifies performed under (role, id) and how many of
// them were rejected, while Config.HotKeys (or mbft_set_key_accounting) has
// the counts on; what is not counted: include/minbft_gpu.h.
func (a *Authenticator) KeyUsage(role api.AuthenticationRole, id uint32) (uses, rejects uint64, err error) {
	slot := C.mbft_key_slot(a.ctx, C.uint32_t(roleByte(role)), C.uint32_t(id))
	if slot < 0 {
		return 0, 0, a.failure("mbft_key_slot", int(slot))
	}
	s := C.uint32_t(slot)
	var u, r C.uint64_t
	if rc := C.mbft_key_usage(a.ctx, &s, 1, &u, &r); rc != C.MBFT_OK {
		return 0, 0, a.failure("mbft_key_usage", int(rc))
	}
	return uint64(u), uint64(r), nil
}

// PromoteHotKeys re-classes the maxKeys most used keys of a class cheaper
// than cls with at least minUses uses into cls (mbft_promote_hot_keys) and
// returns how many.
func (a *Authenticator) PromoteHotKeys(cls uint32, maxKeys int, minUses uint64) (int, error) {
	var n C.size_t
	rc := C.mbft_promote_hot_keys(a.ctx, C.uint32_t(cls), C.size_t(maxKeys), C.uint64_t(minUses), &n)
	if rc != C.MBFT_OK {
		return 0, a.failure("mbft_promote_hot_keys", int(rc))
	}
	return int(n), nil
}

// promoteTick counts a batch (VerifyBatch, CheckMessages) and runs the
// Config.HotKeys promotion every PromoteEvery of them.  A failed promotion
// leaves every key as it was; its error is kept for LastPromoteError.
func (a *Authenticator) promoteTick() {
	if a.hot.PromoteEvery <= 0 {
		return
	}
	if atomic.AddUint64(&a.batches, 1)%uint64(a.hot.PromoteEvery) != 0 {
		return
	}
	if _, err := a.PromoteHotKeys(a.hot.Class, a.hot.MaxKeys, a.hot.MinUses); err != nil {
		a.promoteErr.Store(err.Error())
	} else {
		a.promoteErr.Store("")
	}
}

// LastPromoteError reports the failure of the most recent Config.HotKeys
// promotion, nil if it worked or none has run yet.
func (a *Authenticator) LastPromoteError() error {
	if s, ok := a.promoteErr.Load().(string); ok && s != "" {
		return fmt.Errorf("%s", s)
	}
	return nil
}

// RebalanceResult is what a rebalance did (mbft_rebalance_result).
type RebalanceResult struct {
	LiveBefore, LiveAfter uint64 // bytes of live key data
	PinnedBytes           uint64 // valid keys outside the ladder
	OverBudget            uint64 // bytes past the budget with every ladder key at the first rung
	Promoted, Demoted     int
	KeysPerRung           []int // afterwards, one entry per rung of the ladder
}

// SetKeyBudget sets the bytes of live key data per engine a rebalance plans
// against (mbft_set_key_budget); 0 is none.
func (a *Authenticator) SetKeyBudget(bytes uint64) error {
	if rc := C.mbft_set_key_budget(a.ctx, C.uint64_t(bytes)); rc != C.MBFT_OK {
		return a.failure("mbft_set_key_budget", int(rc))
	}
	return nil
}

// RebalanceKeys gives every key whose class is a rung of ladder the rung of
// its use count within the budget (mbft_rebalance_keys): it demotes and
// promotes.  After a failure part way the result says what was done.
func (a *Authenticator) RebalanceKeys(ladder []uint32, minUses uint64) (RebalanceResult, error) {
	var res C.mbft_rebalance_result
	lad := make([]C.uint32_t, len(ladder)+1) // (+1: an empty ladder still has an address)
	for i, c := range ladder {
		lad[i] = C.uint32_t(c)
	}
	rc := C.mbft_rebalance_keys(a.ctx, &lad[0], C.size_t(len(ladder)), C.uint64_t(minUses), &res)
	out := RebalanceResult{LiveBefore: uint64(res.live_before), LiveAfter: uint64(res.live_after),
		PinnedBytes: uint64(res.pinned_bytes), OverBudget: uint64(res.over_budget),
		Promoted: int(res.promoted), Demoted: int(res.demoted)}
	for i := 0; i < len(ladder) && i < len(res.keys_per_rung); i++ {
		out.KeysPerRung = append(out.KeysPerRung, int(res.keys_per_rung[i]))
	}
	if rc != C.MBFT_OK {
		return out, a.failure("mbft_rebalance_keys", int(rc))
	}
	return out, nil
}

// AgeKeyUsage shifts every use count right by shift bits (mbft_age_key_usage).
func (a *Authenticator) AgeKeyUsage(shift uint) error {
	if rc := C.mbft_age_key_usage(a.ctx, C.uint(shift)); rc != C.MBFT_OK {
		return a.failure("mbft_age_key_usage", int(rc))
	}
	return nil
}

// ColdKeys returns the lowest max key slots whose summed uses are <= maxUses,
// ascending, and how many such slots there are in all (mbft_cold_keys).
func (a *Authenticator) ColdKeys(maxUses uint64, max int) ([]uint32, int, error) {
	if max < 0 {
		max = 0
	}
	buf := make([]C.uint32_t, max+1)
	var n C.size_t
	if rc := C.mbft_cold_keys(a.ctx, C.uint64_t(maxUses), &buf[0], C.size_t(max), &n); rc != C.MBFT_OK {
		return nil, 0, a.failure("mbft_cold_keys", int(rc))
	}
	got := int(n)
	if got > max {
		got = max
	}
	out := make([]uint32, got)
	for i := range out {
		out[i] = uint32(buf[i])
	}
	return out, int(n), nil
}

// evictBatch bounds the client keys one rebalance tick removes.
const evictBatch = 4096

// evictCold removes the client keys the registry maps among the cold slots
// (fewer than Config.KeyBudget.EvictMaxUses uses).  With Config.KeyStore set
// such a key comes back through ensureKey on its next call.
func (a *Authenticator) evictCold() error {
	cold, _, err := a.ColdKeys(a.budget.EvictMaxUses-1, evictBatch)
	if err != nil || len(cold) == 0 {
		return err
	}
	a.keys.mu.RLock()
	var gone []uint32
	for k := range a.keys.known {
		if k.role != api.ClientAuthen {
			continue
		}
		slot := C.mbft_key_slot(a.ctx, C.uint32_t(roleByte(k.role)), C.uint32_t(k.id))
		if slot < 0 {
			continue
		}
		i := sort.Search(len(cold), func(i int) bool { return cold[i] >= uint32(slot) })
		if i < len(cold) && cold[i] == uint32(slot) {
			gone = append(gone, k.id)
		}
	}
	a.keys.mu.RUnlock()
	for _, id := range gone {
		if err := a.RemoveKey(api.ClientAuthen, id); err != nil {
			return err
		}
	}
	return nil
}

// rebalanceTick counts a batch (VerifyBatch, CheckMessages) and, every
// Config.KeyBudget.Every of them, rebalances the keys within the budget,
// then ages the use counts, then evicts cold client keys.  A failure ends the
// tick; its error is kept for LastRebalanceError.
func (a *Authenticator) rebalanceTick() {
	if a.budget.Every <= 0 {
		return
	}
	if atomic.AddUint64(&a.rebalTicks, 1)%uint64(a.budget.Every) != 0 {
		return
	}
	_, err := a.RebalanceKeys(a.budget.Ladder, a.budget.MinUses)
	if err == nil && a.budget.AgeShift > 0 {
		err = a.AgeKeyUsage(a.budget.AgeShift)
	}
	if err == nil && a.budget.EvictMaxUses > 0 {
		err = a.evictCold()
	}
	if err != nil {
		a.rebalErr.Store(err.Error())
	} else {
		a.rebalErr.Store("")
	}
}

// LastRebalanceError reports the failure of the most recent Config.KeyBudget
// tick, nil if it worked or none has run yet.
func (a *Authenticator) LastRebalanceError() error {
	if s, ok := a.rebalErr.Load().(string); ok && s != "" {
		return fmt.Errorf("%s", s)
	}
	return nil
}
