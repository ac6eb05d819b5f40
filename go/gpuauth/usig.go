package gpuauth

// A software USIG on the GPU (Config.GPUUSIG): usig.USIG -- CreateUI,
// VerifyUI, ID -- plus the batch CreateUIs, over the library's
// mbft_usig_* entry points (include/minbft_gpu.h; DESIGN.md §4.6).  What it
// replaces: the SGX USIG (usig/sgx/sgx-usig.go:42-79 New / CreateUI /
// VerifyUI / ID over the enclave's ecall_usig_create_ui,
// usig/sgx/enclave/usig.c:36-76) on hosts that have no SGX -- an MI355X host
// is an EPYC machine.  One UI per PREPARE (primary) or COMMIT (backup), in
// strict counter order.
//
// NO TRUSTED HARDWARE.  MinBFT's f < n/2 bound rests on a USIG that a faulty
// replica cannot make sign twice under one counter.  This one keeps its key
// and counter in ordinary process and device memory: whoever controls the
// host controls them.  It is the equivalent of the SGX SDK's simulation mode
// (the reference CI's SGX_MODE=SIM), for development, tests and benchmarks.
// It is OFF unless Config.GPUUSIG is set, and a deployment that needs the
// fault bound keeps the SGX USIG (Config.Generator / Config.USIGGenerator).
//
// What is kept from the enclave: the epoch is drawn at random when the
// instance starts (crypto/rand here, sgx_read_rand there, usig.c:177-184) and
// is fixed for its life; the counter starts at 1 and moves only when valid
// UIs are handed out; a restart is a new epoch.  UIs are byte-compatible:
// Cert = epoch_be64 || asn1.Marshal{R, S} over SHA256(SHA256(m) || epoch_le ||
// counter_le) (sgx-usig.go:99-101,143-168), so the reference's VerifyUI and
// this library's USIG-role verifier accept them.  The nonce is RFC 6979.

/*
#include "minbft_gpu.h"
*/
import "C"

import (
	"crypto/ecdsa"
	"crypto/rand"
	"crypto/x509"
	"encoding/binary"
	"fmt"
	"unsafe"

	"github.com/hyperledger-labs/minbft/api"
	"github.com/hyperledger-labs/minbft/usig"
)

// uiSlot is MBFT_UI_SLOT, usigIDLen MBFT_USIG_ID_LEN.
const (
	uiSlot    = 88
	usigIDLen = 99
)

// USIG is the context's software USIG instance.
type USIG struct {
	a  *Authenticator
	id []byte // epoch_be64 || PKIX(public key) (sgx-usig.go:105-123 MakeID)
}

var _ usig.USIG = (*USIG)(nil)

// startUSIG makes the instance from Config.PrivateKeys[api.USIGAuthen] with
// a fresh random epoch.  Called by New when Config.GPUUSIG is set.
func (a *Authenticator) startUSIG() error {
	sk := a.priv[api.USIGAuthen]
	if sk == nil {
		return fmt.Errorf("Config.GPUUSIG needs Config.PrivateKeys[api.USIGAuthen]")
	}
	var d [32]byte
	if !put32(d[:], sk.D) {
		return fmt.Errorf("USIG private key: not a P-256 scalar")
	}
	var eb [8]byte
	if _, err := rand.Read(eb[:]); err != nil {
		return fmt.Errorf("USIG epoch: %v", err)
	}
	rc := C.mbft_usig_init(a.ctx, (*C.uint8_t)(unsafe.Pointer(&d[0])), C.uint64_t(binary.BigEndian.Uint64(eb[:])))
	for i := range d {
		d[i] = 0
	}
	if rc != C.MBFT_OK {
		return a.failure("mbft_usig_init", int(rc))
	}
	id := make([]byte, usigIDLen)
	var n C.size_t
	if rc := C.mbft_usig_id(a.ctx, ptr(id), C.size_t(len(id)), &n); rc != C.MBFT_OK {
		return a.failure("mbft_usig_id", int(rc))
	}
	a.usig = &USIG{a: a, id: id[:int(n)]}
	return nil
}

// USIG returns the software USIG, or nil when Config.GPUUSIG is off.
func (a *Authenticator) USIG() *USIG { return a.usig }

// ID implements usig.USIG.
func (u *USIG) ID() []byte { return append([]byte(nil), u.id...) }

// CreateUI implements usig.USIG: the next counter value, bound to message.
func (u *USIG) CreateUI(message []byte) (*usig.UI, error) {
	uis, err := u.CreateUIs([][]byte{message})
	if err != nil {
		return nil, err
	}
	return uis[0], nil
}

// CreateUIs creates one UI per message in one GPU call: uis[i] is bound to
// messages[i] and carries the counter of uis[0] plus i.  Concurrent calls are
// serialised by the library; each gets a contiguous range.  On an error no UI
// was created and the counter has not moved.
func (u *USIG) CreateUIs(messages [][]byte) ([]*usig.UI, error) {
	n := len(messages)
	if n == 0 {
		return nil, nil
	}
	total := 0
	for _, m := range messages {
		total += len(m)
	}
	if n > maxRecs || uint64(total) > 0xFFFFFFFF {
		return nil, fmt.Errorf("CreateUIs: batch of %d messages, %d bytes: too large", n, total)
	}
	// pointer-free Go slices, passed as arguments and not retained
	buf := make([]byte, 0, total+1)
	off := make([]uint32, n+1)
	for i, m := range messages {
		buf = append(buf, m...)
		off[i+1] = uint32(len(buf))
	}
	buf = append(buf, 0)
	slots := make([]byte, uiSlot*n)
	lens := make([]byte, n)
	var first C.uint64_t
	rc := C.mbft_usig_create_uis_flat(u.a.ctx, ptr(buf), u32p(off), C.size_t(n), ptr(slots), ptr(lens), &first)
	if rc != C.MBFT_OK {
		return nil, u.a.failure("mbft_usig_create_uis_flat", int(rc))
	}
	out := make([]*usig.UI, n)
	for i := range out {
		l := int(lens[i])
		ui := slots[i*uiSlot : i*uiSlot+l]
		if l < 16 || binary.BigEndian.Uint64(ui[:8]) != uint64(first)+uint64(i) {
			return nil, fmt.Errorf("CreateUIs: malformed UI %d from the library", i)
		}
		out[i] = &usig.UI{Counter: uint64(first) + uint64(i), Cert: append([]byte(nil), ui[8:]...)}
	}
	return out, nil
}

// VerifyUI implements usig.USIG through the GPU verifier: usigID names the
// epoch and the public key (sgx-usig.go:81-97,125-141); the key must be one
// of the USIGAuthen keys the authenticator was built over, and the UI is then
// checked by VerifyMessageAuthenTag in the USIG role (epoch rule of
// crypto.go:219-236 included).
func (u *USIG) VerifyUI(message []byte, ui *usig.UI, usigID []byte) error {
	if len(usigID) < 8 {
		return fmt.Errorf("invalid USIG ID")
	}
	pub, err := x509.ParsePKIXPublicKey(usigID[8:])
	if err != nil {
		return fmt.Errorf("invalid USIG ID: %v", err)
	}
	pk, ok := pub.(*ecdsa.PublicKey)
	if !ok {
		return fmt.Errorf("invalid USIG ID: not an ECDSA key")
	}
	if len(ui.Cert) < 8 || binary.BigEndian.Uint64(ui.Cert[:8]) != binary.BigEndian.Uint64(usigID[:8]) {
		return fmt.Errorf("epoch value mismatch")
	}
	for id, k := range u.a.usigKeys {
		if k != nil && k.X.Cmp(pk.X) == 0 && k.Y.Cmp(pk.Y) == 0 {
			return u.a.VerifyMessageAuthenTag(api.USIGAuthen, id, message, usig.MustMarshalUI(ui))
		}
	}
	return fmt.Errorf("USIG ID names no known USIG key")
}
