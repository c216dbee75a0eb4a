package gpdecode

// The tcpassembly hand-off (include/gpd_tcpassembly.h) from Go.  Not compiled here (no Go
// toolchain); tests/test_tcpassembly_gpu.py drives the same C entry point through ctypes on the
// GPU.

/*
#cgo CFLAGS: -I${SRCDIR}/../../include -I/opt/rocm/include -D__HIP_PLATFORM_AMD__
#cgo LDFLAGS: -L/opt/rocm/lib -lamdhip64
#include <hip/hip_runtime_api.h>
#include "gpd.h"
#include "gpd_flow.h"
#include "gpd_tcpassembly.h"
*/
import "C"

import (
	"errors"
	"runtime"
	"time"
	"unsafe"

	"github.com/google/gopacket"
	"github.com/google/gopacket/layers"
	"github.com/google/gopacket/tcpassembly"
)

// TCP flag bits of Segment.Flags (header bytes 12..13 & 0x1FF).
const (
	TCPFin = 1 << iota
	TCPSyn
	TCPRst
	TCPPsh
	TCPAck
	TCPUrg
	TCPEce
	TCPCwr
	TCPNs
)

// TCPUngrouped is the flow id of the trailing group: segments whose key got no flow record.
const TCPUngrouped = C.GPD_TCP_UNGROUPED

// Segment is one packet Assembler.AssembleWithTimestamp acts on (C.gpd_tcp_seg).
type Segment struct {
	Packet     uint32 // index in the batch
	FlowID     uint32 // the flow table's record of key{netFlow, t.TransportFlow()}
	Seq, Ack   uint32
	PayloadOff uint32 // t.Payload = packet[PayloadOff : PayloadOff+PayloadLen]
	PayloadLen uint32
	TCPOff     uint16
	Flags      uint16
	LookupOnly bool   // the call would not create a connection (assembly.go:550-551)
	NetOff     uint16 // the header NetworkFlow() reads (the header offsets word's low half, gpd.h)
	NetType    uint8  // its EndpointType as the status word has it: 1 IPv4, 2 IPv6
}

// SegmentGroup is a run of segments with one key: Segments[Start : Start+Count].
type SegmentGroup struct {
	FlowID      uint32 // TCPUngrouped for the tail
	Start       uint32
	Count       uint32
	FirstPacket uint32
}

// Segments is the hand-off of one batch: the segments ordered by flow record and, within one
// record, by packet; Groups describes the runs.
type Segments struct {
	Segments  []Segment
	Groups    []SegmentGroup
	Ungrouped int // segments of the last group when it is the TCPUngrouped tail
}

// Segments decodes the batch on the device, inserts it into the flow table and returns the
// packets Assembler.AssembleWithTimestamp does not ignore (assembly.go:535), grouped by
// connection key:
//
//	ft, _ := p.NewFlowTable(1 << 20)
//	segs, _ := p.Segments(ft, &b)
//	for _, g := range segs.Groups {            // groups are independent: one goroutine each
//	    segs.AssembleGroup(assembler, g, &b, ts)
//	}
//
// The packets of one key stay in capture order, the assembler's one rule; the TCPUngrouped tail
// (keys the full table gave no record) is in packet order and goes to one assembler.
func (p *BatchDecodingLayerParser) Segments(t *FlowTable, b *PacketBatch) (*Segments, error) {
	n := len(b.Offset)
	if n == 0 || len(b.Data) == 0 {
		return &Segments{}, nil
	}
	if t == nil || t.parser != p {
		return nil, errors.New("gpdecode: Segments needs a flow table of this parser")
	}
	if err := p.configure(); err != nil {
		return nil, err
	}
	done, err := p.onDevice()
	if err != nil {
		return nil, err
	}
	defer done()
	// data, offset, caplen, status, layers, hdr_off, flow ids
	sizes := []int{(len(b.Data)+15)&^15 + 64, 4 * n, 4 * n, 4 * n, 8 * n, 4 * n, 4 * n}
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
	in := C.gpd_batch{data: (*C.uint8_t)(bufs[0].p), data_len: C.uint64_t(len(b.Data)),
		offset: (*C.uint32_t)(bufs[1].p), caplen: (*C.uint32_t)(bufs[2].p), n: C.uint64_t(n)}
	res := C.gpd_result{status: (*C.uint32_t)(bufs[3].p), layers: (*C.uint64_t)(bufs[4].p),
		hdr_off: (*C.uint32_t)(bufs[5].p)}
	if rc := C.gpd_decode(p.ctx, &in, &res, nil); rc != C.GPD_OK {
		return nil, lastError("gpd_decode", rc)
	}
	ids := (*C.uint32_t)(bufs[6].p)
	if rc := C.gpd_flow_insert(t.ft, &in, &res, ids, C.uint64_t(t.seq), nil); rc != C.GPD_OK {
		return nil, lastError("gpd_flow_insert", rc)
	}
	t.seq += uint64(n)
	var st C.gpd_flow_stats
	if rc := C.gpd_flow_stats_get(t.ft, &st, nil); rc != C.GPD_OK {
		return nil, lastError("gpd_flow_stats_get", rc)
	}
	bound := C.uint32_t(st.capacity)
	var cnt, ng, un C.uint64_t
	// the sizing call, then the hand-off into arrays of exactly that size
	if rc := C.gpd_tcp_segments(p.ctx, &in, &res, ids, bound, nil, nil, 0, &cnt, &ng, &un, nil); rc != C.GPD_OK {
		return nil, lastError("gpd_tcp_segments", rc)
	}
	if cnt == 0 {
		return &Segments{}, nil
	}
	dseg, err := devAlloc(32 * int(cnt))
	if err != nil {
		return nil, err
	}
	defer dseg.free()
	dgrp, err := devAlloc(16 * int(cnt))
	if err != nil {
		return nil, err
	}
	defer dgrp.free()
	if rc := C.gpd_tcp_segments(p.ctx, &in, &res, ids, bound, (*C.gpd_tcp_seg)(dseg.p), (*C.gpd_tcp_group)(dgrp.p),
		cnt, &cnt, &ng, &un, nil); rc != C.GPD_OK {
		return nil, lastError("gpd_tcp_segments", rc)
	}
	cs := make([]C.gpd_tcp_seg, int(cnt))
	cg := make([]C.gpd_tcp_group, int(ng))
	// the decode's status and header-offset words: where each segment's network header sits
	status, hdrOff := make([]uint32, n), make([]uint32, n)
	if e := C.hipMemcpy(unsafe.Pointer(&status[0]), bufs[3].p, C.size_t(4*n), C.hipMemcpyDeviceToHost); e != C.hipSuccess {
		return nil, errors.New(C.GoString(C.hipGetErrorString(e)))
	}
	if e := C.hipMemcpy(unsafe.Pointer(&hdrOff[0]), bufs[5].p, C.size_t(4*n), C.hipMemcpyDeviceToHost); e != C.hipSuccess {
		return nil, errors.New(C.GoString(C.hipGetErrorString(e)))
	}
	if e := C.hipMemcpy(unsafe.Pointer(&cs[0]), dseg.p, C.size_t(32*int(cnt)), C.hipMemcpyDeviceToHost); e != C.hipSuccess {
		return nil, errors.New(C.GoString(C.hipGetErrorString(e)))
	}
	if e := C.hipMemcpy(unsafe.Pointer(&cg[0]), dgrp.p, C.size_t(16*int(ng)), C.hipMemcpyDeviceToHost); e != C.hipSuccess {
		return nil, errors.New(C.GoString(C.hipGetErrorString(e)))
	}
	out := &Segments{Segments: make([]Segment, len(cs)), Groups: make([]SegmentGroup, len(cg)), Ungrouped: int(un)}
	for k := range cs {
		c := &cs[k]
		out.Segments[k] = Segment{Packet: uint32(c.packet), FlowID: uint32(c.flow_id), Seq: uint32(c.seq),
			Ack: uint32(c.ack), PayloadOff: uint32(c.payload_off), PayloadLen: uint32(c.payload_len),
			TCPOff: uint16(c.tcp_off), Flags: uint16(c.flags), LookupOnly: c.lookup_only != 0,
			NetOff: uint16(hdrOff[c.packet] & 0xFFFF), NetType: uint8(status[c.packet] >> 20 & 15)}
	}
	for k := range cg {
		c := &cg[k]
		out.Groups[k] = SegmentGroup{FlowID: uint32(c.flow_id), Start: uint32(c.start), Count: uint32(c.count),
			FirstPacket: uint32(c.first_packet)}
	}
	runtime.KeepAlive(b)
	return out, nil
}

// AssembleGroup feeds one group to a tcpassembly.Assembler, in the group's order (capture
// order within a key).  The TCP layer is decoded from the segment's own bytes, header through
// payload: DecodeFromBytes fills the private port slices TransportFlow() reads (tcp.go:235,
// 331-333; assigning SrcPort / DstPort alone would leave them nil and give every connection
// between two hosts one key), Seq, the flags, and Payload as the batch decode left it, since the
// slice ends where the record says t.Payload ends.  The network flow is read at the network
// header the decode located (NetOff, NetType); ts[i] is packet i's timestamp.  One layers.TCP is
// reused: the assembler copies what it keeps (pagesFromTCP, assembly.go:734-756).  Groups share
// no key, so each may run on its own goroutine with its own Assembler, over one StreamPool or
// one pool each.  A segment whose bytes do not decode again (none should: the batch decode
// accepted them) is skipped.
func (s *Segments) AssembleGroup(a *tcpassembly.Assembler, g SegmentGroup, b *PacketBatch, ts []time.Time) {
	var t layers.TCP
	for k := g.Start; k < g.Start+g.Count; k++ {
		seg := &s.Segments[k]
		pkt := b.Data[b.Offset[seg.Packet] : b.Offset[seg.Packet]+b.CapLen[seg.Packet]]
		if err := t.DecodeFromBytes(pkt[seg.TCPOff:seg.PayloadOff+seg.PayloadLen], gopacket.NilDecodeFeedback); err != nil {
			continue
		}
		a.AssembleWithTimestamp(netFlowOf(pkt, seg), &t, ts[seg.Packet])
	}
}

// netFlowOf is NetworkFlow() of the segment's network layer (ip4.go:63-65, ip6.go:49-51), read
// at the offset and with the endpoint type the decode reported for it: the same bytes the flow
// table keyed the packet by, whatever lies between that header and the TCP header.
func netFlowOf(pkt []byte, seg *Segment) gopacket.Flow {
	o := int(seg.NetOff)
	if seg.NetType == 1 {
		return gopacket.NewFlow(layers.EndpointIPv4, pkt[o+12:o+16], pkt[o+16:o+20])
	}
	return gopacket.NewFlow(layers.EndpointIPv6, pkt[o+8:o+24], pkt[o+24:o+40])
}
