package gpdecode

// TCP connection tracking (include/gpd_tcptrack.h) from Go: reassembly's bidirectional
// connection, each packet's TCPFlowDirection and the TCPSimpleFSM verdict, one state machine per
// connection kept on the device from batch to batch.  Not compiled here (no Go toolchain);
// tests/test_tcptrack_gpu.py drives the same C entry points through ctypes on the GPU.

/*
#cgo CFLAGS: -I${SRCDIR}/../../include -I/opt/rocm/include -D__HIP_PLATFORM_AMD__
#cgo LDFLAGS: -L/opt/rocm/lib -lamdhip64
#include <hip/hip_runtime_api.h>
#include "gpd.h"
#include "gpd_flow.h"
#include "gpd_tcptrack.h"
*/
import "C"

import (
	"runtime"
	"unsafe"

	"github.com/google/gopacket/reassembly"
)

// Verdict is one packet's byte of ConnTracker.TrackBatch.
type Verdict uint8

// Untracked is the verdict of a packet the tracker does not track (not TCP, no key, no record).
const Untracked Verdict = C.GPD_TCP_UNTRACKED

// Tracked reports whether the packet belongs to a tracked connection.
func (v Verdict) Tracked() bool { return v != Untracked }

// Accept is TCPSimpleFSM.CheckState's result (true for untracked packets: nothing rejects them).
func (v Verdict) Accept() bool { return v == Untracked || v&C.GPD_TCP_V_ACCEPT != 0 }

// Dir is the packet's direction in its connection.
func (v Verdict) Dir() reassembly.TCPFlowDirection {
	if v&C.GPD_TCP_V_DIR != 0 {
		return reassembly.TCPDirServerToClient
	}
	return reassembly.TCPDirClientToServer
}

// State is the connection's state after the packet (reassembly.TCPStateClosed ... TCPStateReset).
func (v Verdict) State() int { return int(v&C.GPD_TCP_V_STATE_MASK) >> C.GPD_TCP_V_STATE_SHIFT }

// StateName is TCPSimpleFSM.String() for a state number.
func StateName(state int) string {
	names := [...]string{"Closed", "SynSent", "Established", "CloseWait", "LastAck", "Reset"}
	if state < 0 || state >= len(names) {
		return "?"
	}
	return names[state]
}

// Tracked is what one batch gave.
type Tracked struct {
	Verdict []Verdict
	ConnID  []uint32 // the connection's flow record (the direction seen first); FlowNone when untracked
	// packets tracked, accepted, rejected; connections that had a packet
	NTracked, Accepted, Rejected, Connections uint64
}

// Keep is the mask Select and the writers take: the accepted packets and, with untracked, the
// packets the tracker does not track.
func (r *Tracked) Keep(untracked bool) []bool {
	keep := make([]bool, len(r.Verdict))
	for i, v := range r.Verdict {
		keep[i] = (v.Tracked() && v.Accept()) || (!v.Tracked() && untracked)
	}
	return keep
}

// ConnTracker is a reassembly.StreamPool of connections over a flow table, each with a
// reassembly.TCPSimpleFSM.
type ConnTracker struct {
	p     *BatchDecodingLayerParser
	t     *FlowTable
	h     *C.gpd_tcp_tracker
	bound uint32
}

// NewConnTracker makes the tracker for the connections the flow table keys; opts are the
// options every connection's reassembly.NewTCPSimpleFSM gets.
func (t *FlowTable) NewConnTracker(opts reassembly.TCPSimpleFSMOptions) (*ConnTracker, error) {
	p := t.parser
	if err := p.configure(); err != nil {
		return nil, err
	}
	var fst C.gpd_flow_stats
	if rc := C.gpd_flow_stats_get(t.ft, &fst, nil); rc != C.GPD_OK {
		return nil, lastError("gpd_flow_stats_get", rc)
	}
	o := C.gpd_tcp_track_opts{}
	if opts.SupportMissingEstablishment {
		o.support_missing_establishment = 1
	}
	var h *C.gpd_tcp_tracker
	if rc := C.gpd_tcp_tracker_create(p.ctx, t.ft, &o, &h); rc != C.GPD_OK {
		return nil, lastError("gpd_tcp_tracker_create", rc)
	}
	return &ConnTracker{p: p, t: t, h: h, bound: uint32(fst.capacity)}, nil
}

// Close frees the tracker.  Call it before the flow table's and the parser's Close.
func (c *ConnTracker) Close() {
	if c.h != nil {
		C.gpd_tcp_tracker_destroy(c.h)
		c.h = nil
	}
}

// Reset returns every connection to the fresh state; call it when the flow table is reset.
func (c *ConnTracker) Reset() error {
	if rc := C.gpd_tcp_tracker_reset(c.h, nil); rc != C.GPD_OK {
		return lastError("gpd_tcp_tracker_reset", rc)
	}
	return nil
}

// Forget returns the listed connections (Tracked.ConnID values) to the fresh state.
func (c *ConnTracker) Forget(ids []uint32) error {
	if len(ids) == 0 {
		return nil
	}
	done, err := c.p.onDevice()
	if err != nil {
		return err
	}
	defer done()
	d, err := devAlloc(4 * len(ids))
	if err != nil {
		return err
	}
	defer d.free()
	if err := toDev(d, unsafe.Pointer(&ids[0]), 4*len(ids)); err != nil {
		return err
	}
	if rc := C.gpd_tcp_tracker_forget(c.h, (*C.uint32_t)(d.p), C.uint64_t(len(ids)), nil); rc != C.GPD_OK {
		return lastError("gpd_tcp_tracker_forget", rc)
	}
	if rc := C.hipDeviceSynchronize(); rc != 0 {
		return lastError("hipDeviceSynchronize", C.GPD_ERR_HIP)
	}
	return nil
}

// States returns the carried byte of every flow record: the state in bits 0..2 and the FSM's
// direction in bit 3, on the connection's own record.
func (c *ConnTracker) States() ([]uint8, error) {
	if c.bound == 0 {
		return nil, nil
	}
	done, err := c.p.onDevice()
	if err != nil {
		return nil, err
	}
	defer done()
	d, err := devAlloc(int(c.bound))
	if err != nil {
		return nil, err
	}
	defer d.free()
	if rc := C.gpd_tcp_tracker_states(c.h, (*C.uint8_t)(d.p), nil); rc != C.GPD_OK {
		return nil, lastError("gpd_tcp_tracker_states", rc)
	}
	out := make([]uint8, c.bound)
	if err := fromDev(unsafe.Pointer(&out[0]), d, int(c.bound)); err != nil {
		return nil, err
	}
	return out, nil
}

// TrackBatch decodes the batch on the device, keys it with the flow table and steps every TCP
// connection's state machine with its packets in capture order.
//
//	tr, _ := table.NewConnTracker(reassembly.TCPSimpleFSMOptions{})
//	for b := range batches {
//	    r, _ := tr.TrackBatch(&b)
//	    kept, index, _ := p.Select(&b, r.Keep(true)) // what Stream.Accept would have let through
//	}
func (c *ConnTracker) TrackBatch(b *PacketBatch) (*Tracked, error) {
	p, t := c.p, c.t
	n := len(b.Offset)
	if n == 0 || len(b.Data) == 0 {
		return &Tracked{}, nil
	}
	done, err := p.onDevice()
	if err != nil {
		return nil, err
	}
	defer done()
	// data, offset, caplen, status, layers, hdr_off, flow ids, verdicts, connection ids
	sizes := []int{(len(b.Data)+15)&^15 + 64, 4 * n, 4 * n, 4 * n, 8 * n, 4 * n, 4 * n, n + 16, 4 * n}
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
	t.seq += uint64(n) // (grows from call to call: a connection's direction, once fixed, stays)
	var tot [4]C.uint64_t
	if rc := C.gpd_tcp_tracker_run(c.h, &in, &res, ids, (*C.uint8_t)(bufs[7].p), (*C.uint32_t)(bufs[8].p), &tot[0],
		nil); rc != C.GPD_OK {
		return nil, lastError("gpd_tcp_tracker_run", rc)
	}
	out := &Tracked{Verdict: make([]Verdict, n), ConnID: make([]uint32, n), NTracked: uint64(tot[0]),
		Accepted: uint64(tot[1]), Rejected: uint64(tot[2]), Connections: uint64(tot[3])}
	if err := fromDev(unsafe.Pointer(&out.Verdict[0]), bufs[7], n); err != nil {
		return nil, err
	}
	if err := fromDev(unsafe.Pointer(&out.ConnID[0]), bufs[8], 4*n); err != nil {
		return nil, err
	}
	runtime.KeepAlive(b)
	return out, nil
}
