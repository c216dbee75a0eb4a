package gpdecode

// BPF filtering of a batch on the device (include/gpd_bpf.h) from Go.  Not compiled here (no Go
// toolchain); tests/test_bpf_gpu.py drives the same C entry points through ctypes on the GPU and
// tests/c/bpf_host.c the host ones from plain C.

/*
#cgo CFLAGS: -I${SRCDIR}/../../include -I/opt/rocm/include -D__HIP_PLATFORM_AMD__
#cgo LDFLAGS: -L/opt/rocm/lib -lamdhip64
#include <hip/hip_runtime_api.h>
#include "gpd.h"
#include "gpd_bpf.h"
*/
import "C"

import (
	"errors"
	"runtime"
	"unsafe"

	"github.com/google/gopacket"
)

// MaxBpfInstructions is pcap.MaxBpfInstructions (pcap/pcap.go:36).
const MaxBpfInstructions = 4096

// BPFInstruction is pcap.BPFInstruction (pcap/pcap.go:113-119); a []pcap.BPFInstruction converts
// element by element.
type BPFInstruction struct {
	Code uint16
	Jt   uint8
	Jf   uint8
	K    uint32
}

// BPF is pcap.BPF (pcap/pcap.go:553-583) over the parser's device context.
type BPF struct {
	p    *BatchDecodingLayerParser
	prog []C.gpd_bpf_insn
	f    *C.gpd_bpf
}

func cProgram(insns []BPFInstruction) []C.gpd_bpf_insn {
	prog := make([]C.gpd_bpf_insn, len(insns))
	for i, q := range insns {
		prog[i] = C.gpd_bpf_insn{code: C.uint16_t(q.Code), jt: C.uint8_t(q.Jt), jf: C.uint8_t(q.Jf), k: C.uint32_t(q.K)}
	}
	return prog
}

func progPtr(prog []C.gpd_bpf_insn) *C.gpd_bpf_insn {
	if len(prog) == 0 {
		return nil
	}
	return &prog[0]
}

// ValidateBPF is the check NewBPFInstructionFilter makes, without a device: the length rule of
// pcap/pcap.go:504-511 and the instruction rules of include/gpd_bpf.h.
func ValidateBPF(insns []BPFInstruction) error {
	prog := cProgram(insns)
	if rc := C.gpd_bpf_validate(progPtr(prog), C.uint32_t(len(prog))); rc != C.GPD_OK {
		return lastError("gpd_bpf_validate", rc)
	}
	return nil
}

// NewBPFInstructionFilter is pcap.NewBPFInstructionFilter (pcap/pcap.go:553-570): the program is
// validated and uploaded to the parser's device.  Close releases it (the finalizer does too).
func (p *BatchDecodingLayerParser) NewBPFInstructionFilter(insns []BPFInstruction) (*BPF, error) {
	if err := p.configure(); err != nil {
		return nil, err
	}
	b := &BPF{p: p, prog: cProgram(insns)}
	if rc := C.gpd_bpf_create(p.ctx, progPtr(b.prog), C.uint32_t(len(b.prog)), &b.f); rc != C.GPD_OK {
		return nil, lastError("gpd_bpf_create", rc)
	}
	runtime.SetFinalizer(b, (*BPF).Close)
	return b, nil
}

// Close frees the device copy of the program; it must run before the parser is closed.
func (b *BPF) Close() {
	if b.f != nil {
		C.gpd_bpf_destroy(b.f)
		b.f = nil
	}
}

// String is (*BPF).String (pcap/pcap.go:576-578).
func (b *BPF) String() string { return "BPF Instruction Filter" }

// Matches is (*BPF).Matches (pcap/pcap.go:581-583) for one host packet, through the interpreter
// the device runs, compiled for the host.  Unlike the reference it accepts an empty packet.
func (b *BPF) Matches(ci gopacket.CaptureInfo, data []byte) bool {
	return C.gpd_bpf_run_host(progPtr(b.prog), C.uint32_t(len(b.prog)), (*C.uint8_t)(bytesPtr(data)),
		C.uint32_t(len(data)), C.uint32_t(ci.Length)) != 0
}

// MatchBatch is the loop
//
//	for i := range keep { keep[i] = f.Matches(ci[i], b.Packet(i)) }
//
// run on the device; the result is what WritePackets and Select take.  ci may be nil: Length is
// then each packet's capture length.
func (b *BPF) MatchBatch(pb *PacketBatch, ci []gopacket.CaptureInfo) ([]bool, error) {
	n := len(pb.Offset)
	keep := make([]bool, n)
	if n == 0 {
		return keep, nil
	}
	if ci != nil && len(ci) < n {
		return nil, errors.New("gpdecode: MatchBatch needs a CaptureInfo per packet (or none)")
	}
	p := b.p
	done, err := p.onDevice()
	if err != nil {
		return nil, err
	}
	defer done()
	in, _, free, err := p.upload(pb, nil)
	defer free()
	if err != nil {
		return nil, err
	}
	var dwl devBuf
	if ci != nil {
		wl := make([]uint32, n)
		for i := range wl {
			wl[i] = uint32(ci[i].Length)
		}
		if dwl, err = devAlloc(4 * n); err != nil {
			return nil, err
		}
		defer dwl.free()
		if err := toDev(dwl, unsafe.Pointer(&wl[0]), 4*n); err != nil {
			return nil, err
		}
	}
	dkeep, err := devAlloc(n)
	if err != nil {
		return nil, err
	}
	defer dkeep.free()
	if rc := C.gpd_bpf_filter(b.f, &in, (*C.uint32_t)(dwl.p), (*C.uint8_t)(dkeep.p), nil, nil); rc != C.GPD_OK {
		return nil, lastError("gpd_bpf_filter", rc)
	}
	host := make([]byte, n)
	// (hipMemcpy on the null stream waits for the filter queued on it)
	if e := C.hipMemcpy(unsafe.Pointer(&host[0]), dkeep.p, C.size_t(n), C.hipMemcpyDeviceToHost); e != C.hipSuccess {
		return nil, errors.New(C.GoString(C.hipGetErrorString(e)))
	}
	for i, v := range host {
		keep[i] = v != 0
	}
	runtime.KeepAlive(pb)
	return keep, nil
}
