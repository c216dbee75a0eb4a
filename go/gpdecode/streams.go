package gpdecode

// TCP stream assembly (include/gpd_tcpstream.h) from Go: the Reassembly lists of a batch's
// connections, built on the device, delivered into real tcpassembly.Streams.  Not compiled here
// (no Go toolchain); tests/test_tcpstream_gpu.py drives the same C entry point through ctypes on
// the GPU.

/*
#cgo CFLAGS: -I${SRCDIR}/../../include -I/opt/rocm/include -D__HIP_PLATFORM_AMD__
#cgo LDFLAGS: -L/opt/rocm/lib -lamdhip64
#include <hip/hip_runtime_api.h>
#include "gpd.h"
#include "gpd_flow.h"
#include "gpd_tcpassembly.h"
#include "gpd_tcpstream.h"
*/
import "C"

import (
	"errors"
	"runtime"
	"time"
	"unsafe"

	"github.com/google/gopacket"
	"github.com/google/gopacket/tcpassembly"
)

// Flag bits of StreamRecord.Flags.
const (
	ReasmStart   = C.GPD_TCP_R_START
	ReasmEnd     = C.GPD_TCP_R_END
	ReasmFlushed = C.GPD_TCP_R_FLUSHED // the call was made by the end-of-batch drain (skipFlush)
)

// StreamOptions are the assembler's options gpd_tcp_assemble offers.  MaxBufferedPagesTotal is
// not among them: it couples all connections through one page counter.
type StreamOptions struct {
	MaxBufferedPagesPerConnection int  // AssemblerOptions.MaxBufferedPagesPerConnection; 0: none
	CloseAll                      bool // FlushAll's close after the drain
	NoGather                      bool // records only: Bytes are sliced out of the batch in place
}

// StreamRecord is one Reassembly handed to Stream.Reassembled (C.gpd_tcp_reasm).
type StreamRecord struct {
	Packet    uint32 // the packet the bytes come from; Reassembly.Seen is its timestamp
	SrcOff    uint32 // offset of Bytes[0] in that packet
	Len       uint32
	Skip      int32
	StreamOff uint64 // offset of Bytes in Streams.Bytes
	Call      uint32 // records with one Call form one Reassembled([]Reassembly)
	Flags     uint16
}

// Stream is one assembled connection (C.gpd_tcp_stream).
type Stream struct {
	FlowID, FirstRec, NRec, NCalls uint32
	ByteOff, NBytes                uint64
	Completed                      uint32 // ReassemblyComplete calls for this key in this batch
	Open                           bool   // still in the pool afterwards
	NextSeq                        uint32
}

// Streams is the assembly of one batch.
type Streams struct {
	Records []StreamRecord
	Streams []Stream
	Bytes   []byte // every stream's bytes back to back; nil with NoGather
	Calls   uint64
}

// ConnState carries the open connections of a flow table from batch to batch: 8 bytes per flow
// record on the device.  Make a new one when the table is reset.
type ConnState struct {
	buf   devBuf
	bound uint32
}

// NewConnState allocates the zeroed state for a flow table.
func (t *FlowTable) NewConnState() (*ConnState, error) {
	var st C.gpd_flow_stats
	if rc := C.gpd_flow_stats_get(t.ft, &st, nil); rc != C.GPD_OK {
		return nil, lastError("gpd_flow_stats_get", rc)
	}
	d, err := devAlloc(8 * int(st.capacity))
	if err != nil {
		return nil, err
	}
	if e := C.hipMemset(d.p, 0, C.size_t(8*int(st.capacity))); e != C.hipSuccess {
		d.free()
		return nil, errors.New(C.GoString(C.hipGetErrorString(e)))
	}
	return &ConnState{buf: d, bound: uint32(st.capacity)}, nil
}

// Close frees the state.
func (s *ConnState) Close() { s.buf.free() }

func fromDev(dst unsafe.Pointer, src devBuf, n int) error {
	if n == 0 {
		return nil
	}
	if e := C.hipMemcpy(dst, src.p, C.size_t(n), C.hipMemcpyDeviceToHost); e != C.hipSuccess {
		return errors.New(C.GoString(C.hipGetErrorString(e)))
	}
	return nil
}

// Streams decodes the batch on the device, inserts it into the flow table, groups its TCP
// segments by connection (gpd_tcp_segments) and assembles every group (gpd_tcp_assemble): for
// each key AssembleWithTimestamp per segment, then the drain of what is still buffered (a batch
// is the reordering horizon), then with CloseAll the close of what is still open.  state may be
// nil: every connection then starts and ends with the batch.
//
//	ft, _ := p.NewFlowTable(1 << 20)
//	st, _ := ft.NewConnState()
//	for b := range batches {
//	    s, _ := p.Streams(ft, st, &b, gpdecode.StreamOptions{})
//	    s.Deliver(factory, live, keyOf, &b, ts)
//	}
func (p *BatchDecodingLayerParser) Streams(t *FlowTable, state *ConnState, b *PacketBatch, opt StreamOptions) (*Streams, error) {
	n := len(b.Offset)
	if n == 0 || len(b.Data) == 0 {
		return &Streams{}, nil
	}
	if t == nil || t.parser != p {
		return nil, errors.New("gpdecode: Streams needs a flow table of this parser")
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
	var fst C.gpd_flow_stats
	if rc := C.gpd_flow_stats_get(t.ft, &fst, nil); rc != C.GPD_OK {
		return nil, lastError("gpd_flow_stats_get", rc)
	}
	bound := C.uint32_t(fst.capacity)
	var cnt, ng, un C.uint64_t
	if rc := C.gpd_tcp_segments(p.ctx, &in, &res, ids, bound, nil, nil, 0, &cnt, &ng, &un, nil); rc != C.GPD_OK {
		return nil, lastError("gpd_tcp_segments", rc)
	}
	if cnt == 0 {
		return &Streams{}, nil
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
	segs, groups := (*C.gpd_tcp_seg)(dseg.p), (*C.gpd_tcp_group)(dgrp.p)
	if rc := C.gpd_tcp_segments(p.ctx, &in, &res, ids, bound, segs, groups, cnt, &cnt, &ng, &un, nil); rc != C.GPD_OK {
		return nil, lastError("gpd_tcp_segments", rc)
	}
	// the assembly: the sizing call, then arrays of exactly that size
	o := C.gpd_tcp_asm_opts{max_pages_per_connection: C.uint32_t(opt.MaxBufferedPagesPerConnection)}
	if opt.CloseAll {
		o.close_all = 1
	}
	var cstate *C.gpd_tcp_conn
	var sbound C.uint32_t
	if state != nil {
		cstate, sbound = (*C.gpd_tcp_conn)(state.buf.p), C.uint32_t(state.bound)
	}
	var tot [4]C.uint64_t
	if rc := C.gpd_tcp_assemble(p.ctx, &in, segs, cnt, groups, ng, cstate, sbound, &o, nil, 0, nil, nil, 0,
		&tot[0], nil); rc != C.GPD_OK {
		return nil, lastError("gpd_tcp_assemble", rc)
	}
	nrec, nbytes := int(tot[0]), int(tot[2])
	drec, err := devAlloc(32*nrec + 32)
	if err != nil {
		return nil, err
	}
	defer drec.free()
	dstr, err := devAlloc(48 * int(ng))
	if err != nil {
		return nil, err
	}
	defer dstr.free()
	var dbytes devBuf
	var bp *C.uint8_t
	var mb C.uint64_t
	if !opt.NoGather {
		if dbytes, err = devAlloc(nbytes + 16); err != nil {
			return nil, err
		}
		defer dbytes.free()
		bp, mb = (*C.uint8_t)(dbytes.p), C.uint64_t(nbytes)
	}
	if rc := C.gpd_tcp_assemble(p.ctx, &in, segs, cnt, groups, ng, cstate, sbound, &o, (*C.gpd_tcp_reasm)(drec.p),
		C.uint64_t(nrec), (*C.gpd_tcp_stream)(dstr.p), bp, mb, &tot[0], nil); rc != C.GPD_OK {
		return nil, lastError("gpd_tcp_assemble", rc)
	}
	nstr := int(tot[1])
	cr := make([]C.gpd_tcp_reasm, nrec+1)
	cs := make([]C.gpd_tcp_stream, nstr+1)
	if err := fromDev(unsafe.Pointer(&cr[0]), drec, 32*nrec); err != nil {
		return nil, err
	}
	if err := fromDev(unsafe.Pointer(&cs[0]), dstr, 48*nstr); err != nil {
		return nil, err
	}
	out := &Streams{Records: make([]StreamRecord, nrec), Streams: make([]Stream, nstr), Calls: uint64(tot[3])}
	if !opt.NoGather {
		out.Bytes = make([]byte, nbytes+1)[:nbytes]
		if nbytes > 0 {
			if err := fromDev(unsafe.Pointer(&out.Bytes[0]), dbytes, nbytes); err != nil {
				return nil, err
			}
		}
	}
	for k := 0; k < nrec; k++ {
		c := &cr[k]
		out.Records[k] = StreamRecord{Packet: uint32(c.packet), SrcOff: uint32(c.src_off), Len: uint32(c.len),
			Skip: int32(c.skip), StreamOff: uint64(c.stream_off), Call: uint32(c.call), Flags: uint16(c.flags)}
	}
	for k := 0; k < nstr; k++ {
		c := &cs[k]
		out.Streams[k] = Stream{FlowID: uint32(c.flow_id), FirstRec: uint32(c.first_rec), NRec: uint32(c.nrec),
			NCalls: uint32(c.ncalls), ByteOff: uint64(c.byte_off), NBytes: uint64(c.nbytes),
			Completed: uint32(c.completed), Open: c.open != 0, NextSeq: uint32(c.next_seq)}
	}
	runtime.KeepAlive(b)
	return out, nil
}

// Deliver makes the calls the reference's assembler makes, stream by stream: factory.New for a
// key that has no stream in `live` yet (keyOf gives the network and transport flows of a flow
// record, e.g. from FlowTable.Export), Reassembled per call, ReassemblyComplete after a call
// whose last Reassembly has End and for FlushAll's close.  live keeps the streams of connections
// that stay open between batches, as the StreamPool does.  b and ts are the batch and its
// timestamps (Reassembly.Seen; b also supplies the bytes when nothing was gathered).
func (s *Streams) Deliver(factory tcpassembly.StreamFactory, live map[uint32]tcpassembly.Stream,
	keyOf func(flowID uint32) (net, transport gopacket.Flow), b *PacketBatch, ts []time.Time) {
	var call []tcpassembly.Reassembly
	for i := range s.Streams {
		st := &s.Streams[i]
		if st.NCalls == 0 && st.Completed == 0 {
			continue
		}
		stream := live[st.FlowID]
		open := func() {
			if stream == nil {
				stream = factory.New(keyOf(st.FlowID))
				live[st.FlowID] = stream
			}
		}
		ended := uint32(0)
		recs := s.Records[st.FirstRec : st.FirstRec+st.NRec]
		for k := 0; k < len(recs); {
			e := k
			call = call[:0]
			for ; e < len(recs) && recs[e].Call == recs[k].Call; e++ {
				r := &recs[e]
				var bytes []byte
				if s.Bytes != nil {
					bytes = s.Bytes[r.StreamOff : r.StreamOff+uint64(r.Len)]
				} else {
					at := b.Offset[r.Packet] + r.SrcOff
					bytes = b.Data[at : at+r.Len]
				}
				call = append(call, tcpassembly.Reassembly{Bytes: bytes, Skip: int(r.Skip),
					Start: r.Flags&ReasmStart != 0, End: r.Flags&ReasmEnd != 0, Seen: ts[r.Packet]})
			}
			open()
			stream.Reassembled(call)
			if call[len(call)-1].End {
				stream.ReassemblyComplete()
				delete(live, st.FlowID)
				stream = nil
				ended++
			}
			k = e
		}
		if st.Completed > ended { // still open after the drain, closed by CloseAll
			open()
			stream.ReassemblyComplete()
			delete(live, st.FlowID)
		}
	}
}
