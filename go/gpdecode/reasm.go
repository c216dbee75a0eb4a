package gpdecode

// IPv4 defragmentation (include/gpd_ip4reasm.h) from Go: ip4defrag's datagrams rebuilt on the
// device, the unfinished fragment lists kept there from batch to batch.  Not compiled here (no Go
// toolchain); tests/test_ip4reasm_gpu.py drives the same C entry points through ctypes on the GPU.

/*
#cgo CFLAGS: -I${SRCDIR}/../../include -I/opt/rocm/include -D__HIP_PLATFORM_AMD__
#cgo LDFLAGS: -L/opt/rocm/lib -lamdhip64
#include <hip/hip_runtime_api.h>
#include "gpd.h"
#include "gpd_defrag.h"
#include "gpd_ip4reasm.h"
*/
import "C"

import (
	"errors"
	"fmt"
	"runtime"
	"time"
	"unsafe"
)

// What DefragIPv4WithTimestamp returned for one handed-over packet (FragOutcome.What).
const (
	FragFiled     = C.GPD_IP4_FILED     // (nil, nil)
	FragComplete  = C.GPD_IP4_COMPLETE  // (out, nil): Datagram indexes Defragmented.Datagrams
	FragRejected  = C.GPD_IP4_REJECTED  // securityChecks
	FragUnchanged = C.GPD_IP4_UNCHANGED // (in, nil)
	FragHole      = C.GPD_IP4_HOLE
	FragInvalid   = C.GPD_IP4_INVALID
	FragListFull  = C.GPD_IP4_LIST_FULL
)

// DatagramShortSlice marks a datagram whose build took Payload[startAt:] past the payload's end
// (Go's ip4defrag panics there; nothing was appended for that fragment).
const DatagramShortSlice = C.GPD_IP4_D_SHORT_SLICE

// FragOutcome is the outcome of one hand-off record (C.gpd_ip4_outcome).
type FragOutcome struct {
	What     uint32
	Datagram uint32
}

// Err is the error DefragIPv4WithTimestamp returns for the outcome, in the reference's words
// (securityChecks' text needs the values of the packet: see the record's verdict).
func (o FragOutcome) Err() error {
	switch o.What {
	case FragRejected:
		return errors.New("defrag: fragment rejected by securityChecks")
	case FragHole:
		return errors.New("defrag: building - hole found")
	case FragInvalid:
		return errors.New("defrag: building - invalid fragment")
	case FragListFull:
		return fmt.Errorf("defrag: Fragment List hits its maximum"+
			"size(%d), without success. Flushing the list", int(C.GPD_IP4_MAX_LIST_LEN))
	}
	return nil
}

// Datagram is one reassembled datagram (C.gpd_ip4_dgram): the layers.IPv4 build returns.
type Datagram struct {
	Packet     uint32 // the completing packet
	Frag       uint32 // its index among the handed-over packets
	ByteOff    uint64 // the datagram in Defragmented.Bytes: 4*IHL header bytes, then the payload
	PayloadLen uint32
	NFrags     uint32
	Length     uint16 // out.Length = Highest
	Id         uint16
	IHL        uint8
	Protocol   uint8
	Flags      uint16
}

// Defragmented is what one batch's fragments gave.
type Defragmented struct {
	Packets   []uint32      // the handed-over packets, in packet order
	Outcomes  []FragOutcome // one per handed-over packet
	Datagrams []Datagram
	Batch     PacketBatch // the datagrams as a batch to decode with first layer IPv4
	Lists     uint64      // fragment lists held afterwards
}

// IPv4Defragmenter is ip4defrag.IPv4Defragmenter on the parser's device.
type IPv4Defragmenter struct {
	p *BatchDecodingLayerParser
	d *C.gpd_ip4_defrag
}

// NewIPv4Defragmenter is ip4defrag.NewIPv4Defragmenter.
func (p *BatchDecodingLayerParser) NewIPv4Defragmenter() (*IPv4Defragmenter, error) {
	if err := p.configure(); err != nil {
		return nil, err
	}
	var d *C.gpd_ip4_defrag
	if rc := C.gpd_ip4_defrag_create(p.ctx, &d); rc != C.GPD_OK {
		return nil, lastError("gpd_ip4_defrag_create", rc)
	}
	return &IPv4Defragmenter{p: p, d: d}, nil
}

// Close frees the defragmenter and the fragments it holds.
func (f *IPv4Defragmenter) Close() {
	if f.d != nil {
		C.gpd_ip4_defrag_destroy(f.d)
		f.d = nil
	}
}

// DiscardOlderThan is IPv4Defragmenter.DiscardOlderThan.
func (f *IPv4Defragmenter) DiscardOlderThan(t time.Time) (int, error) {
	var n C.uint64_t
	if rc := C.gpd_ip4_defrag_discard(f.d, C.uint64_t(t.UnixNano()), &n); rc != C.GPD_OK {
		return 0, lastError("gpd_ip4_defrag_discard", rc)
	}
	return int(n), nil
}

// Stats reports the lists, fragments and payload bytes held.
func (f *IPv4Defragmenter) Stats() (lists, fragments, bytes uint64, err error) {
	var o [3]C.uint64_t
	if rc := C.gpd_ip4_defrag_stats(f.d, &o[0]); rc != C.GPD_OK {
		return 0, 0, 0, lastError("gpd_ip4_defrag_stats", rc)
	}
	return uint64(o[0]), uint64(o[1]), uint64(o[2]), nil
}

// DefragBatch decodes the batch on the device, hands its IPv4 fragments over
// (gpd_ip4_fragments) and runs DefragIPv4WithTimestamp for them in packet order
// (gpd_ip4_defrag_run).  ts may be nil: LastSeen is then time.Now().
//
//	d, _ := p.NewIPv4Defragmenter()
//	for b := range batches {
//	    r, _ := d.DefragBatch(&b, ts)
//	    ip4.DecodeBatch(&r.Batch)            // a parser with first layer LayerTypeIPv4
//	}
func (f *IPv4Defragmenter) DefragBatch(b *PacketBatch, ts []time.Time) (*Defragmented, error) {
	p := f.p
	n := len(b.Offset)
	if n == 0 || len(b.Data) == 0 {
		return &Defragmented{}, nil
	}
	done, err := p.onDevice()
	if err != nil {
		return nil, err
	}
	defer done()
	// data, offset, caplen, status, layers, hdr_off, timestamps
	sizes := []int{(len(b.Data)+15)&^15 + 64, 4 * n, 4 * n, 4 * n, 8 * n, 4 * n, 8 * n}
	bufs := make([]devBuf, len(sizes))
	for k, s := range sizes {
		d, err := devAlloc(s)
		if err != nil {
			return nil, err
		}
		bufs[k] = d
		defer d.free()
	}
	if err := toDev(bufs[0], unsafe.Pointer(&b.Data[0]), len(b.Data)); err != nil {
		return nil, err
	}
	if err := toDev(bufs[1], unsafe.Pointer(&b.Offset[0]), 4*n); err != nil {
		return nil, err
	}
	if err := toDev(bufs[2], unsafe.Pointer(&b.CapLen[0]), 4*n); err != nil {
		return nil, err
	}
	var dts *C.uint64_t
	if ts != nil {
		if len(ts) < n {
			return nil, errors.New("gpdecode: DefragBatch needs a timestamp per packet")
		}
		ns := make([]uint64, n)
		for i := range ns {
			ns[i] = uint64(ts[i].UnixNano())
		}
		if err := toDev(bufs[6], unsafe.Pointer(&ns[0]), 8*n); err != nil {
			return nil, err
		}
		dts = (*C.uint64_t)(bufs[6].p)
	}
	in := C.gpd_batch{data: (*C.uint8_t)(bufs[0].p), data_len: C.uint64_t(len(b.Data)),
		offset: (*C.uint32_t)(bufs[1].p), caplen: (*C.uint32_t)(bufs[2].p), n: C.uint64_t(n)}
	res := C.gpd_result{status: (*C.uint32_t)(bufs[3].p), layers: (*C.uint64_t)(bufs[4].p),
		hdr_off: (*C.uint32_t)(bufs[5].p)}
	if rc := C.gpd_decode(p.ctx, &in, &res, nil); rc != C.GPD_OK {
		return nil, lastError("gpd_decode", rc)
	}
	var cnt C.uint64_t
	if rc := C.gpd_ip4_fragments(p.ctx, &in, &res, nil, 0, &cnt, nil); rc != C.GPD_OK {
		return nil, lastError("gpd_ip4_fragments", rc)
	}
	if cnt == 0 {
		return &Defragmented{}, nil
	}
	nf := int(cnt)
	dfr, err := devAlloc(32 * nf)
	if err != nil {
		return nil, err
	}
	defer dfr.free()
	frags := (*C.gpd_ip4_frag)(dfr.p)
	if rc := C.gpd_ip4_fragments(p.ctx, &in, &res, frags, cnt, &cnt, nil); rc != C.GPD_OK {
		return nil, lastError("gpd_ip4_fragments", rc)
	}
	now := C.uint64_t(time.Now().UnixNano())
	// the sizing call, then arrays of exactly that size
	var tot [4]C.uint64_t
	if rc := C.gpd_ip4_defrag_run(f.d, &in, frags, cnt, dts, now, nil, nil, 0, nil, nil, nil, 0, &tot[0], nil); rc != C.GPD_OK {
		return nil, lastError("gpd_ip4_defrag_run", rc)
	}
	nd, nb := int(tot[0]), int(tot[2])
	m := (nd + 15) &^ 15
	out := []int{8*nf + 16, 32*nd + 32, 4*m + 64, 4*m + 64, nb + 16}
	ob := make([]devBuf, len(out))
	for k, s := range out {
		d, err := devAlloc(s)
		if err != nil {
			return nil, err
		}
		ob[k] = d
		defer d.free()
	}
	if rc := C.gpd_ip4_defrag_run(f.d, &in, frags, cnt, dts, now, (*C.gpd_ip4_outcome)(ob[0].p),
		(*C.gpd_ip4_dgram)(ob[1].p), C.uint64_t(nd), (*C.uint32_t)(ob[2].p), (*C.uint32_t)(ob[3].p),
		(*C.uint8_t)(ob[4].p), C.uint64_t(nb), &tot[0], nil); rc != C.GPD_OK {
		return nil, lastError("gpd_ip4_defrag_run", rc)
	}
	cf := make([]C.gpd_ip4_frag, nf)
	co := make([]C.gpd_ip4_outcome, nf)
	cd := make([]C.gpd_ip4_dgram, nd+1)
	if err := fromDev(unsafe.Pointer(&cf[0]), dfr, 32*nf); err != nil {
		return nil, err
	}
	if err := fromDev(unsafe.Pointer(&co[0]), ob[0], 8*nf); err != nil {
		return nil, err
	}
	if err := fromDev(unsafe.Pointer(&cd[0]), ob[1], 32*nd); err != nil {
		return nil, err
	}
	r := &Defragmented{Packets: make([]uint32, nf), Outcomes: make([]FragOutcome, nf),
		Datagrams: make([]Datagram, nd), Lists: uint64(tot[3])}
	for k := 0; k < nf; k++ {
		r.Packets[k] = uint32(cf[k].packet)
		r.Outcomes[k] = FragOutcome{What: uint32(co[k].what), Datagram: uint32(co[k].datagram)}
	}
	for k := 0; k < nd; k++ {
		c := &cd[k]
		r.Datagrams[k] = Datagram{Packet: uint32(c.packet), Frag: uint32(c.frag), ByteOff: uint64(c.byte_off),
			PayloadLen: uint32(c.payload_len), NFrags: uint32(c.nfrags), Length: uint16(c.length), Id: uint16(c.id),
			IHL: uint8(c.ihl), Protocol: uint8(c.protocol), Flags: uint16(c.flags)}
	}
	if nd > 0 {
		r.Batch = PacketBatch{Data: make([]byte, nb+64)[:nb], Offset: make([]uint32, nd), CapLen: make([]uint32, nd)}
		if err := fromDev(unsafe.Pointer(&r.Batch.Offset[0]), ob[2], 4*nd); err != nil {
			return nil, err
		}
		if err := fromDev(unsafe.Pointer(&r.Batch.CapLen[0]), ob[3], 4*nd); err != nil {
			return nil, err
		}
		if nb > 0 {
			if err := fromDev(unsafe.Pointer(&r.Batch.Data[0]), ob[4], nb); err != nil {
				return nil, err
			}
		}
	}
	runtime.KeepAlive(b)
	return r, nil
}
