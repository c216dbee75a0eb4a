package gpdecode

// The stateful TCP assembler (include/gpd_tcpasm.h) from Go: tcpassembly's Assembler + StreamPool
// as a device object that keeps out-of-order data, nextSeq and lastSeen per flow record from batch
// to batch, with FlushWithOptions / FlushOlderThan / FlushAll.  Not compiled here (no Go
// toolchain); tests/test_tcpasm_gpu.py drives the same C entry points through ctypes on the GPU.

/*
#cgo CFLAGS: -I${SRCDIR}/../../include -I/opt/rocm/include -D__HIP_PLATFORM_AMD__
#cgo LDFLAGS: -L/opt/rocm/lib -lamdhip64
#include <hip/hip_runtime_api.h>
#include "gpd.h"
#include "gpd_flow.h"
#include "gpd_tcpassembly.h"
#include "gpd_tcpstream.h"
#include "gpd_tcpasm.h"
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

// Further flag bits of StreamRecord.Flags and of AssembledStream.Open.
const (
	ReasmCarried = C.GPD_TCP_R_CARRIED // the bytes come from a page carried from an earlier batch
	ConnOpen     = C.GPD_TCP_CONN_OPEN
	ConnNoSeq    = C.GPD_TCP_CONN_NOSEQ // nextSeq is invalidSequence
	NoPacket     = C.GPD_TCP_NO_PACKET  // StreamRecord.Packet of a carried record
)

// AssembledStream is one stream record of a run (C.gpd_tcp_stream as gpd_tcp_assembler_run fills it).
type AssembledStream struct {
	FlowID, FirstRec, NRec, NCalls uint32
	ByteOff, NBytes                uint64
	Completed                      uint32 // ReassemblyComplete calls for this key in this run
	Open                           uint32 // ConnOpen | ConnNoSeq afterwards
	NextSeq                        uint32
	Pages                          uint32 // pages the connection still buffers
}

// Assembled is what one run gave.
type Assembled struct {
	Records []StreamRecord
	Seen    []time.Time // Reassembly.Seen per record
	Streams []AssembledStream
	Bytes   []byte
	Calls   uint64
	// held afterwards
	Connections, Pages, PageBytes uint64
	// flow ids open before the run: Deliver calls StreamFactory.New for the others only
	OpenBefore map[uint32]bool
}

// ConnInfo is one connection the assembler holds (C.gpd_tcp_conn_info).
type ConnInfo struct {
	NextSeq, Flags, Pages, PageBytes uint32
	LastSeen                         time.Time
}

// Assembler is tcpassembly.Assembler with its StreamPool on the parser's device.
type Assembler struct {
	p     *BatchDecodingLayerParser
	t     *FlowTable
	a     *C.gpd_tcp_assembler
	bound uint32
}

// NewAssembler is tcpassembly.NewAssembler(tcpassembly.NewStreamPool(...)) for the connections
// the flow table keys.  maxPagesPerConnection is AssemblerOptions.MaxBufferedPagesPerConnection
// (0: none); MaxBufferedPagesTotal is not offered.
func (t *FlowTable) NewAssembler(maxPagesPerConnection int) (*Assembler, error) {
	p := t.parser
	if err := p.configure(); err != nil {
		return nil, err
	}
	var fst C.gpd_flow_stats
	if rc := C.gpd_flow_stats_get(t.ft, &fst, nil); rc != C.GPD_OK {
		return nil, lastError("gpd_flow_stats_get", rc)
	}
	o := C.gpd_tcp_asm_opts{max_pages_per_connection: C.uint32_t(maxPagesPerConnection)}
	var a *C.gpd_tcp_assembler
	if rc := C.gpd_tcp_assembler_create(p.ctx, C.uint32_t(fst.capacity), &o, &a); rc != C.GPD_OK {
		return nil, lastError("gpd_tcp_assembler_create", rc)
	}
	return &Assembler{p: p, t: t, a: a, bound: uint32(fst.capacity)}, nil
}

// Close frees the assembler and the pages it holds.  Call it before the parser's Close.
func (a *Assembler) Close() {
	if a.a != nil {
		C.gpd_tcp_assembler_destroy(a.a)
		a.a = nil
	}
}

// Reset drops every connection; call it when the flow table is reset.
func (a *Assembler) Reset() error {
	if rc := C.gpd_tcp_assembler_reset(a.a, nil); rc != C.GPD_OK {
		return lastError("gpd_tcp_assembler_reset", rc)
	}
	return nil
}

// Stats reports the connections, connections with pages, pages and page bytes held.
func (a *Assembler) Stats() (conns, withPages, pages, pageBytes uint64, err error) {
	var o [4]C.uint64_t
	if rc := C.gpd_tcp_assembler_stats(a.a, &o[0]); rc != C.GPD_OK {
		return 0, 0, 0, 0, lastError("gpd_tcp_assembler_stats", rc)
	}
	return uint64(o[0]), uint64(o[1]), uint64(o[2]), uint64(o[3]), nil
}

// Conns returns the connections held, by flow id (a zero Flags: none).
func (a *Assembler) Conns() ([]ConnInfo, error) {
	if a.bound == 0 {
		return nil, nil
	}
	done, err := a.p.onDevice()
	if err != nil {
		return nil, err
	}
	defer done()
	d, err := devAlloc(24 * int(a.bound))
	if err != nil {
		return nil, err
	}
	defer d.free()
	if rc := C.gpd_tcp_assembler_conns(a.a, (*C.gpd_tcp_conn_info)(d.p), nil); rc != C.GPD_OK {
		return nil, lastError("gpd_tcp_assembler_conns", rc)
	}
	c := make([]C.gpd_tcp_conn_info, a.bound)
	if err := fromDev(unsafe.Pointer(&c[0]), d, 24*int(a.bound)); err != nil {
		return nil, err
	}
	out := make([]ConnInfo, a.bound)
	for k := range c {
		out[k] = ConnInfo{NextSeq: uint32(c[k].next_seq), Flags: uint32(c[k].flags), Pages: uint32(c[k].pages),
			PageBytes: uint32(c[k].page_bytes), LastSeen: time.Unix(0, int64(c[k].last_seen_ns))}
	}
	return out, nil
}

func (a *Assembler) openBefore() (map[uint32]bool, error) {
	open := map[uint32]bool{}
	n, _, _, _, err := a.Stats()
	if err != nil || n == 0 {
		return open, err
	}
	cs, err := a.Conns()
	if err != nil {
		return nil, err
	}
	for k, c := range cs {
		if c.Flags&ConnOpen != 0 {
			open[uint32(k)] = true
		}
	}
	return open, nil
}

// run is gpd_tcp_assembler_run: the sizing call, arrays of exactly that size, the run, the copies.
func (a *Assembler) run(in *C.gpd_batch, segs *C.gpd_tcp_seg, cnt C.uint64_t, groups *C.gpd_tcp_group, ng C.uint64_t,
	dts *C.uint64_t, fl C.gpd_tcp_flush) (*Assembled, error) {
	open, err := a.openBefore()
	if err != nil {
		return nil, err
	}
	now := C.uint64_t(time.Now().UnixNano())
	var tot [8]C.uint64_t
	if rc := C.gpd_tcp_assembler_run(a.a, in, segs, cnt, groups, ng, dts, now, &fl, nil, 0, nil, nil, 0, nil, 0,
		&tot[0], nil); rc != C.GPD_OK {
		return nil, lastError("gpd_tcp_assembler_run", rc)
	}
	nrec, nstr, nbytes := int(tot[0]), int(tot[1]), int(tot[2])
	sizes := []int{32*nrec + 32, 8*nrec + 16, 48*nstr + 48, nbytes + 16}
	ob := make([]devBuf, len(sizes))
	for k, s := range sizes {
		d, err := devAlloc(s)
		if err != nil {
			return nil, err
		}
		ob[k] = d
		defer d.free()
	}
	if rc := C.gpd_tcp_assembler_run(a.a, in, segs, cnt, groups, ng, dts, now, &fl, (*C.gpd_tcp_reasm)(ob[0].p),
		C.uint64_t(nrec), (*C.uint64_t)(ob[1].p), (*C.gpd_tcp_stream)(ob[2].p), C.uint64_t(nstr),
		(*C.uint8_t)(ob[3].p), C.uint64_t(nbytes), &tot[0], nil); rc != C.GPD_OK {
		return nil, lastError("gpd_tcp_assembler_run", rc)
	}
	cr := make([]C.gpd_tcp_reasm, nrec+1)
	cn := make([]uint64, nrec+1)
	cs := make([]C.gpd_tcp_stream, nstr+1)
	if err := fromDev(unsafe.Pointer(&cr[0]), ob[0], 32*nrec); err != nil {
		return nil, err
	}
	if err := fromDev(unsafe.Pointer(&cn[0]), ob[1], 8*nrec); err != nil {
		return nil, err
	}
	if err := fromDev(unsafe.Pointer(&cs[0]), ob[2], 48*nstr); err != nil {
		return nil, err
	}
	out := &Assembled{Records: make([]StreamRecord, nrec), Seen: make([]time.Time, nrec),
		Streams: make([]AssembledStream, nstr), Bytes: make([]byte, nbytes+1)[:nbytes], Calls: uint64(tot[3]),
		Connections: uint64(tot[4]), Pages: uint64(tot[5]), PageBytes: uint64(tot[6]), OpenBefore: open}
	if nbytes > 0 {
		if err := fromDev(unsafe.Pointer(&out.Bytes[0]), ob[3], nbytes); err != nil {
			return nil, err
		}
	}
	for k := 0; k < nrec; k++ {
		c := &cr[k]
		out.Records[k] = StreamRecord{Packet: uint32(c.packet), SrcOff: uint32(c.src_off), Len: uint32(c.len),
			Skip: int32(c.skip), StreamOff: uint64(c.stream_off), Call: uint32(c.call), Flags: uint16(c.flags)}
		out.Seen[k] = time.Unix(0, int64(cn[k]))
	}
	for k := 0; k < nstr; k++ {
		c := &cs[k]
		out.Streams[k] = AssembledStream{FlowID: uint32(c.flow_id), FirstRec: uint32(c.first_rec), NRec: uint32(c.nrec),
			NCalls: uint32(c.ncalls), ByteOff: uint64(c.byte_off), NBytes: uint64(c.nbytes),
			Completed: uint32(c.completed), Open: uint32(c.open), NextSeq: uint32(c.next_seq), Pages: uint32(c.reserved)}
	}
	return out, nil
}

// FlushWithOptions is Assembler.FlushWithOptions over every connection held.
func (a *Assembler) FlushWithOptions(opt tcpassembly.FlushOptions) (*Assembled, error) {
	done, err := a.p.onDevice()
	if err != nil {
		return nil, err
	}
	defer done()
	fl := C.gpd_tcp_flush{}
	if !opt.T.IsZero() {
		fl.before_ns = C.uint64_t(opt.T.UnixNano())
	}
	if opt.CloseAll {
		fl.close_all = 1
	}
	return a.run(nil, nil, 0, nil, 0, nil, fl)
}

// FlushOlderThan is Assembler.FlushOlderThan: FlushWithOptions with CloseAll.
func (a *Assembler) FlushOlderThan(t time.Time) (*Assembled, error) {
	return a.FlushWithOptions(tcpassembly.FlushOptions{T: t, CloseAll: true})
}

// FlushAll is Assembler.FlushAll.
func (a *Assembler) FlushAll() (*Assembled, error) {
	done, err := a.p.onDevice()
	if err != nil {
		return nil, err
	}
	defer done()
	return a.run(nil, nil, 0, nil, 0, nil, C.gpd_tcp_flush{flush_all: 1})
}

// AssembleBatch decodes the batch on the device, keys it with the flow table, hands its TCP
// segments over grouped by connection (gpd_tcp_segments) and runs AssembleWithTimestamp for
// them on top of the connections held, then FlushWithOptions(flush).  ts may be nil: every
// timestamp is then time.Now().
//
//	asm, _ := table.NewAssembler(0)
//	live := map[uint32]tcpassembly.Stream{}
//	for b := range batches {
//	    r, _ := asm.AssembleBatch(&b, ts, tcpassembly.FlushOptions{T: newest.Add(-2 * time.Minute)})
//	    r.Deliver(factory, live, keyOf)
//	}
func (a *Assembler) AssembleBatch(b *PacketBatch, ts []time.Time, flush tcpassembly.FlushOptions) (*Assembled, error) {
	p, t := a.p, a.t
	n := len(b.Offset)
	if n == 0 || len(b.Data) == 0 {
		return a.FlushWithOptions(flush)
	}
	done, err := p.onDevice()
	if err != nil {
		return nil, err
	}
	defer done()
	// data, offset, caplen, status, layers, hdr_off, flow ids, timestamps
	sizes := []int{(len(b.Data)+15)&^15 + 64, 4 * n, 4 * n, 4 * n, 8 * n, 4 * n, 4 * n, 8 * n}
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
			return nil, errors.New("gpdecode: AssembleBatch needs a timestamp per packet")
		}
		ns := make([]uint64, n)
		for i := range ns {
			ns[i] = uint64(ts[i].UnixNano())
		}
		if err := toDev(bufs[7], unsafe.Pointer(&ns[0]), 8*n); err != nil {
			return nil, err
		}
		dts = (*C.uint64_t)(bufs[7].p)
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
	var cnt, ng, un C.uint64_t
	if rc := C.gpd_tcp_segments(p.ctx, &in, &res, ids, C.uint32_t(a.bound), nil, nil, 0, &cnt, &ng, &un, nil); rc != C.GPD_OK {
		return nil, lastError("gpd_tcp_segments", rc)
	}
	fl := C.gpd_tcp_flush{}
	if !flush.T.IsZero() {
		fl.before_ns = C.uint64_t(flush.T.UnixNano())
	}
	if flush.CloseAll {
		fl.close_all = 1
	}
	if cnt == 0 {
		return a.run(nil, nil, 0, nil, 0, nil, fl)
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
	if rc := C.gpd_tcp_segments(p.ctx, &in, &res, ids, C.uint32_t(a.bound), segs, groups, cnt, &cnt, &ng, &un, nil); rc != C.GPD_OK {
		return nil, lastError("gpd_tcp_segments", rc)
	}
	out, err := a.run(&in, segs, cnt, groups, ng, dts, fl)
	runtime.KeepAlive(b)
	return out, err
}

// Deliver makes the calls the reference's assembler makes for one run, stream by stream:
// factory.New for a key that was not open before the run (keyOf gives the network and transport
// flows of a flow record, e.g. from FlowTable.Export), Reassembled per call with Reassembly.Seen
// from Seen, ReassemblyComplete after a call whose last record has End and for a close made by
// a flush.  live is the caller's pool across runs.
func (r *Assembled) Deliver(factory tcpassembly.StreamFactory, live map[uint32]tcpassembly.Stream,
	keyOf func(flowID uint32) (net, transport gopacket.Flow)) {
	fresh := func(key uint32) tcpassembly.Stream {
		n, t := keyOf(key)
		return factory.New(n, t)
	}
	for _, s := range r.Streams {
		key := s.FlowID
		if !r.OpenBefore[key] {
			delete(live, key)
		}
		st := live[key]
		recs := r.Records[s.FirstRec : s.FirstRec+s.NRec]
		seen := r.Seen[s.FirstRec : s.FirstRec+s.NRec]
		ended := uint32(0)
		for k := 0; k < len(recs); {
			e := k
			for e < len(recs) && recs[e].Call == recs[k].Call {
				e++
			}
			call := make([]tcpassembly.Reassembly, 0, e-k)
			for j := k; j < e; j++ {
				c := recs[j]
				call = append(call, tcpassembly.Reassembly{Bytes: r.Bytes[c.StreamOff : c.StreamOff+uint64(c.Len)],
					Skip: int(c.Skip), Start: c.Flags&ReasmStart != 0, End: c.Flags&ReasmEnd != 0, Seen: seen[j]})
			}
			if st == nil {
				st = fresh(key)
				live[key] = st
			}
			st.Reassembled(call)
			if call[len(call)-1].End {
				st.ReassemblyComplete()
				delete(live, key)
				st = nil
				ended++
			}
			k = e
		}
		if s.Completed > ended { // closed by a flush with no data left
			if st == nil {
				st = fresh(key)
			}
			st.ReassemblyComplete()
			delete(live, key)
			st = nil
		}
		if st == nil && s.Open&ConnOpen != 0 && (!r.OpenBefore[key] || s.Completed > 0) {
			live[key] = fresh(key) // created by segments that made no call yet
		}
	}
}
