package gpuauth

// Batch generation on the GPU (Config.GPUGenerate): n calls of
// GenerateMessageAuthenTag for an ECDSA role at once, by the library's
// uniform-access signer (mbft_generate_tags_flat / mbft_sign_messages_flat,
// include/minbft_gpu.h; DESIGN.md §4.5) -- the kernel's memory addresses,
// branches and loop counts do not depend on the key or the nonce, so it is
// fit for the node's real keys.  What it replaces: one REPLY signed per
// executed request (core/utils.go:43-53 through makeGeneratedMessageHandler,
// core/message-handling.go:552-568, ReplicaAuthen) and one REQUEST signed per
// client request (client/request.go:194-204, ClientAuthen).  Tags are
// asn1.Marshal(ecdsaSignature{R, S}) as crypto.go:57-69 makes them, with an
// RFC 6979 nonce where the reference draws from crypto/rand: they verify
// identically.
//
// GenerateMessageAuthenTag itself stays on the CPU (gpuauth.go): a lone call
// is served by Go's signer; USIG UIs stay in the SGX enclave unless
// Config.GPUUSIG starts the software USIG (usig.go).

/*
#include "minbft_gpu.h"
*/
import "C"

import (
	"fmt"
	"unsafe"

	"github.com/hyperledger-labs/minbft/api"
)

// tagSlot is MBFT_TAG_SLOT: the bytes of one tag slot.
const tagSlot = 72

// uploadPrivateKeys hands the ECDSA roles' private keys to the library
// (mbft_set_private_key: a 32-byte device buffer per role, zeroed before it
// is freed).  Called by New when Config.GPUGenerate is set.
func (a *Authenticator) uploadPrivateKeys() error {
	for role, sk := range a.priv {
		if sk == nil || (role != api.ReplicaAuthen && role != api.ClientAuthen) {
			continue
		}
		var d [32]byte
		if !put32(d[:], sk.D) {
			return fmt.Errorf("private key of role %v: not a P-256 scalar", role)
		}
		rc := C.mbft_set_private_key(a.ctx, C.uint32_t(roleByte(role)), (*C.uint8_t)(unsafe.Pointer(&d[0])))
		for i := range d {
			d[i] = 0
		}
		if rc != C.MBFT_OK {
			return a.failure("mbft_set_private_key", int(rc))
		}
	}
	a.gpuGen = true
	return nil
}

// splitTags copies the tags out of their slots.
func splitTags(tags, lens []byte) ([][]byte, error) {
	out := make([][]byte, len(lens))
	for i := range lens {
		l := int(lens[i])
		if l == 0 { // no nonce in 4 candidates: unreachable in practice
			return nil, fmt.Errorf("GPU signer: item %d not signed", i)
		}
		out[i] = append([]byte(nil), tags[i*tagSlot:i*tagSlot+l]...)
	}
	return out, nil
}

// GenerateBatch returns GenerateMessageAuthenTag(role, msgs[i]) for every i,
// signed on the GPU in one call.  role is ReplicaAuthen or ClientAuthen and
// needs its key in Config.PrivateKeys; Config.GPUGenerate must be set.  Only
// the first 32 bytes of each message travel: the scheme's digest is
// (msg || SHA256(""))[0:32] (crypto.go:113-121).
func (a *Authenticator) GenerateBatch(role api.AuthenticationRole, msgs [][]byte) ([][]byte, error) {
	if !a.gpuGen {
		return nil, fmt.Errorf("GPU generation is off (Config.GPUGenerate)")
	}
	n := len(msgs)
	if n == 0 {
		return nil, nil
	}
	// pointer-free Go slices, passed as arguments and not retained
	e := make([]byte, 32*n)
	off := make([]uint32, n+1)
	for i, m := range msgs {
		k := copy(e[32*i:32*i+32], m)
		copy(e[32*i+k:32*i+32], sha256Empty[:])
		off[i+1] = uint32(32 * (i + 1))
	}
	tags := make([]byte, tagSlot*n)
	lens := make([]byte, n)
	rc := C.mbft_generate_tags_flat(a.ctx, C.uint32_t(roleByte(role)), ptr(e), u32p(off), C.size_t(n),
		ptr(tags), ptr(lens))
	if rc != C.MBFT_OK {
		return nil, a.failure("mbft_generate_tags_flat", int(rc))
	}
	return splitTags(tags, lens)
}

// SignMessages signs what the core and the client sign, from the messages'
// raw fields (the records messages.go marshals; Op / result hashed on the
// GPU): REPLY and REQ-VIEW-CHANGE with the replica key, REQUEST with the
// client key.  A PREPARE or COMMIT (USIG UI, SGX) is an error and nothing is
// signed.  tags[i] is the Signature of msgs[i].
func (a *Authenticator) SignMessages(msgs []api.AuthenMessage) ([][]byte, error) {
	if !a.gpuGen {
		return nil, fmt.Errorf("GPU generation is off (Config.GPUGenerate)")
	}
	n := len(msgs)
	if n == 0 {
		return nil, nil
	}
	if n > maxRecs {
		return nil, fmt.Errorf("batch of %d messages: more than %d", n, maxRecs)
	}
	for i := range msgs {
		switch msgs[i].Type {
		case api.AuthenRequest, api.AuthenReply, api.AuthenReqViewChange:
		default:
			return nil, fmt.Errorf("SignMessages: message %d of type %d is not signed by an ECDSA role", i, msgs[i].Type)
		}
	}
	ar := a.arenas.get()
	defer a.arenas.put(ar)
	recs, bytes, nbytes := ar.packMessages(msgs)
	tags := make([]byte, tagSlot*n)
	lens := make([]byte, n)
	rc := C.mbft_sign_messages_flat(a.ctx, recs, C.size_t(n), bytes, C.size_t(nbytes), ptr(tags), ptr(lens))
	if rc != C.MBFT_OK {
		return nil, a.failure("mbft_sign_messages_flat", int(rc))
	}
	return splitTags(tags, lens)
}
