package gpdecode

// The pcap writer and batch selection (include/gpd_pcapwrite.h) and the pcapng writer
// (include/gpd_pcapngwrite.h) from Go.  Not compiled here (no Go toolchain);
// tests/test_pcapwrite_gpu.py and tests/test_pcapngwrite_gpu.py drive the same C entry points
// through ctypes on the GPU.

/*
#cgo CFLAGS: -I${SRCDIR}/../../include -I/opt/rocm/include -D__HIP_PLATFORM_AMD__
#cgo LDFLAGS: -L/opt/rocm/lib -lamdhip64
#include <hip/hip_runtime_api.h>
#include "gpd.h"
#include "gpd_pcap.h"
#include "gpd_pcapwrite.h"
#include "gpd_pcapngwrite.h"
*/
import "C"

import (
	"errors"
	"io"
	"runtime"
	"time"
	"unsafe"

	"github.com/google/gopacket"
	"github.com/google/gopacket/layers"
	"github.com/google/gopacket/pcapgo"
)

// Writer is pcapgo.Writer (pcapgo/write.go:22-129) whose WritePackets takes a whole batch and a
// keep mask and builds the records on the device.
type Writer struct {
	w     io.Writer
	p     *BatchDecodingLayerParser
	nanos bool
}

// NewWriter is pcapgo.NewWriter (write.go:74-76): microsecond timestamps.
func (p *BatchDecodingLayerParser) NewWriter(w io.Writer) *Writer { return &Writer{w: w, p: p} }

// NewWriterNanos is pcapgo.NewWriterNanos (write.go:53-55).
func (p *BatchDecodingLayerParser) NewWriterNanos(w io.Writer) *Writer {
	return &Writer{w: w, p: p, nanos: true}
}

func (w *Writer) flags() C.uint32_t {
	if w.nanos {
		return C.GPD_PCAPW_NANOS
	}
	return 0
}

// WriteFileHeader is Writer.WriteFileHeader (write.go:80-96).
func (w *Writer) WriteFileHeader(snaplen uint32, linktype layers.LinkType) error {
	var buf [24]byte
	if rc := C.gpd_pcap_file_header(w.flags(), C.uint32_t(snaplen), C.uint32_t(linktype), (*C.uint8_t)(&buf[0])); rc != C.GPD_OK {
		return lastError("gpd_pcap_file_header", rc)
	}
	_, err := w.w.Write(buf[:])
	return err
}

// upload puts the batch (and a keep mask, which may be nil: every packet) on the device.
func (p *BatchDecodingLayerParser) upload(b *PacketBatch, keep []bool) (in C.gpd_batch, dkeep devBuf, free func(), err error) {
	n := len(b.Offset)
	var bufs []devBuf
	free = func() {
		for _, d := range bufs {
			d.free()
		}
	}
	alloc := func(size int, src unsafe.Pointer, bytes int) (devBuf, error) {
		d, e := devAlloc(size)
		if e != nil {
			return d, e
		}
		bufs = append(bufs, d)
		return d, toDev(d, src, bytes)
	}
	data, e := alloc((len(b.Data)+15)&^15+64, bytesPtr(b.Data), len(b.Data))
	if e != nil {
		return in, dkeep, free, e
	}
	off, e := alloc(4*n, unsafe.Pointer(&b.Offset[0]), 4*n)
	if e != nil {
		return in, dkeep, free, e
	}
	ln, e := alloc(4*n, unsafe.Pointer(&b.CapLen[0]), 4*n)
	if e != nil {
		return in, dkeep, free, e
	}
	if keep != nil {
		k := make([]byte, n)
		for i, v := range keep {
			if v {
				k[i] = 1
			}
		}
		if dkeep, e = alloc(n, unsafe.Pointer(&k[0]), n); e != nil {
			return in, dkeep, free, e
		}
	}
	in = C.gpd_batch{data: (*C.uint8_t)(data.p), data_len: C.uint64_t(len(b.Data)),
		offset: (*C.uint32_t)(off.p), caplen: (*C.uint32_t)(ln.p), n: C.uint64_t(n)}
	return in, dkeep, free, nil
}

// WritePackets is the loop
//
//	for i := range ci { if keep[i] { err = w.WritePacket(ci[i], b.Packet(i)) } }
//
// run on the device: it returns the records written.  Like the loop it stops at the first kept
// packet with CaptureLength > Length, after writing the records before it.  A zero Timestamp is
// replaced by time.Now() here, as write.go:103-105 does per packet.  keep may be nil.
func (w *Writer) WritePackets(b *PacketBatch, ci []gopacket.CaptureInfo, keep []bool) (int, error) {
	n := len(b.Offset)
	if n == 0 {
		return 0, nil
	}
	if len(ci) < n || (keep != nil && len(keep) < n) {
		return 0, errors.New("gpdecode: WritePackets needs a CaptureInfo (and keep flag) per packet")
	}
	p := w.p
	if err := p.configure(); err != nil {
		return 0, err
	}
	done, err := p.onDevice()
	if err != nil {
		return 0, err
	}
	defer done()
	in, dkeep, free, err := p.upload(b, keep)
	defer free()
	if err != nil {
		return 0, err
	}
	ts, wl := make([]uint64, n), make([]uint32, n)
	for i := range ts {
		t := ci[i].Timestamp
		if t.IsZero() {
			t = time.Now()
		}
		ts[i], wl[i] = uint64(t.UnixNano()), uint32(ci[i].Length)
	}
	dts, err := devAlloc(8 * n)
	if err != nil {
		return 0, err
	}
	defer dts.free()
	dwl, err := devAlloc(4 * n)
	if err != nil {
		return 0, err
	}
	defer dwl.free()
	if err := toDev(dts, unsafe.Pointer(&ts[0]), 8*n); err != nil {
		return 0, err
	}
	if err := toDev(dwl, unsafe.Pointer(&wl[0]), 4*n); err != nil {
		return 0, err
	}
	call := func(out unsafe.Pointer, cap uint64) (C.int, uint64, uint64) {
		var nw, nb, bad C.uint64_t
		rc := C.gpd_pcap_write(p.ctx, &in, (*C.uint64_t)(dts.p), (*C.uint32_t)(dwl.p), (*C.uint8_t)(dkeep.p),
			w.flags(), 0, 0, (*C.uint8_t)(out), C.uint64_t(cap), &nw, &nb, &bad, nil)
		return rc, uint64(nw), uint64(nb)
	}
	rc, _, need := call(nil, 0) // the sizing call
	if rc != C.GPD_OK && rc != C.GPD_ERR_PCAP {
		return 0, lastError("gpd_pcap_write", rc)
	}
	dout, err := devAlloc(int(need))
	if err != nil {
		return 0, err
	}
	defer dout.free()
	rc, nw, nb := call(dout.p, need)
	if rc != C.GPD_OK && rc != C.GPD_ERR_PCAP {
		return 0, lastError("gpd_pcap_write", rc)
	}
	werr := lastError("gpd_pcap_write", rc) // the rejected packet's text; read before any other call
	if nb > 0 {
		host := make([]byte, nb)
		if e := C.hipMemcpy(unsafe.Pointer(&host[0]), dout.p, C.size_t(nb), C.hipMemcpyDeviceToHost); e != C.hipSuccess {
			return 0, errors.New(C.GoString(C.hipGetErrorString(e)))
		}
		if _, err := w.w.Write(host); err != nil {
			return int(nw), err
		}
	}
	runtime.KeepAlive(b)
	if rc == C.GPD_ERR_PCAP {
		return int(nw), werr
	}
	return int(nw), nil
}

// Select returns the packets keep marks as a new batch (16-byte slots) and their indices in b
// (gpd_batch_select), e.g. to decode them again with other decoders, or to hand one flow on.
func (p *BatchDecodingLayerParser) Select(b *PacketBatch, keep []bool) (*PacketBatch, []uint32, error) {
	n := len(b.Offset)
	out := &PacketBatch{}
	if n == 0 {
		return out, nil, nil
	}
	if keep != nil && len(keep) < n {
		return nil, nil, errors.New("gpdecode: Select needs a keep flag per packet")
	}
	if err := p.configure(); err != nil {
		return nil, nil, err
	}
	done, err := p.onDevice()
	if err != nil {
		return nil, nil, err
	}
	defer done()
	in, dkeep, free, err := p.upload(b, keep)
	defer free()
	if err != nil {
		return nil, nil, err
	}
	var k, nb C.uint64_t
	if rc := C.gpd_batch_select(p.ctx, &in, (*C.uint8_t)(dkeep.p), nil, 0, nil, nil, nil, 0, &k, &nb, nil); rc != C.GPD_OK {
		return nil, nil, lastError("gpd_batch_select", rc)
	}
	m, total := int(k), int(nb)
	if m == 0 {
		return out, nil, nil
	}
	sizes := []int{total, 4 * m, 4 * m, 4 * m}
	d := make([]devBuf, len(sizes))
	for j, s := range sizes {
		if d[j], err = devAlloc(s); err != nil {
			return nil, nil, err
		}
		defer d[j].free()
	}
	if rc := C.gpd_batch_select(p.ctx, &in, (*C.uint8_t)(dkeep.p), (*C.uint8_t)(d[0].p), C.uint64_t(total),
		(*C.uint32_t)(d[1].p), (*C.uint32_t)(d[2].p), (*C.uint32_t)(d[3].p), C.uint64_t(m), &k, &nb, nil); rc != C.GPD_OK {
		return nil, nil, lastError("gpd_batch_select", rc)
	}
	if rc := C.gpd_sync(p.ctx, nil); rc != C.GPD_OK {
		return nil, nil, lastError("gpd_sync", rc)
	}
	out.Data = make([]byte, total+64)[:total]
	out.Offset, out.CapLen = make([]uint32, m), make([]uint32, m)
	index := make([]uint32, m)
	for _, c := range []struct {
		dst unsafe.Pointer
		src devBuf
		n   int
	}{{bytesPtr(out.Data), d[0], total}, {unsafe.Pointer(&out.Offset[0]), d[1], 4 * m},
		{unsafe.Pointer(&out.CapLen[0]), d[2], 4 * m}, {unsafe.Pointer(&index[0]), d[3], 4 * m}} {
		if c.n == 0 {
			continue
		}
		if e := C.hipMemcpy(c.dst, c.src.p, C.size_t(c.n), C.hipMemcpyDeviceToHost); e != C.hipSuccess {
			return nil, nil, errors.New(C.GoString(C.hipGetErrorString(e)))
		}
	}
	runtime.KeepAlive(b)
	return out, index, nil
}

// NgWriter is pcapgo.NgWriter (pcapgo/ngwrite.go:45-397) whose WriteBatch takes a whole batch and
// a keep mask and builds the enhanced packet blocks on the device.  The section, interface and
// statistics blocks are built on the host by the library.  Nothing is buffered: there is no Flush.
type NgWriter struct {
	w    io.Writer
	p    *BatchDecodingLayerParser
	intf uint32 // interfaces added so far
}

// ngStrs lays strings back to back and describes them as gpd_pcapng_str.
func ngStrs(vals ...string) ([]byte, []C.gpd_pcapng_str) {
	var buf []byte
	d := make([]C.gpd_pcapng_str, len(vals))
	for i, v := range vals {
		d[i] = C.gpd_pcapng_str{off: C.uint64_t(len(buf)), len: C.uint32_t(len(v))}
		buf = append(buf, v...)
	}
	return buf, d
}

// ngBlock runs a builder twice: the sizing call, then the block.
func ngBlock(what string, build func(out *C.uint8_t, cap C.uint64_t, n *C.uint64_t) C.int) ([]byte, error) {
	var n C.uint64_t
	if rc := build(nil, 0, &n); rc != C.GPD_OK {
		return nil, lastError(what, rc)
	}
	buf := make([]byte, int(n))
	if rc := build((*C.uint8_t)(bytesPtr(buf)), n, &n); rc != C.GPD_OK {
		return nil, lastError(what, rc)
	}
	return buf, nil
}

// NewNgWriterInterface is pcapgo.NewNgWriterInterface (ngwrite.go:66-79): the section header and
// the first interface are written at once.
func (p *BatchDecodingLayerParser) NewNgWriterInterface(w io.Writer, intf pcapgo.NgInterface, options pcapgo.NgWriterOptions) (*NgWriter, error) {
	ret := &NgWriter{w: w, p: p}
	si := options.SectionInfo
	strs, d := ngStrs(si.Hardware, si.OS, si.Application, si.Comment)
	info := C.gpd_pcapng_section_info{hardware: d[0], os: d[1], application: d[2], comment: d[3]}
	block, err := ngBlock("gpd_pcapng_section_block", func(out *C.uint8_t, cap C.uint64_t, n *C.uint64_t) C.int {
		return C.gpd_pcapng_section_block(&info, (*C.uint8_t)(bytesPtr(strs)), C.uint64_t(len(strs)), out, cap, n)
	})
	if err != nil {
		return nil, err
	}
	if _, err := w.Write(block); err != nil {
		return nil, err
	}
	if _, err := ret.AddInterface(intf); err != nil {
		return nil, err
	}
	return ret, nil
}

// NewNgWriter is pcapgo.NewNgWriter (ngwrite.go:56-60).
func (p *BatchDecodingLayerParser) NewNgWriter(w io.Writer, linkType layers.LinkType) (*NgWriter, error) {
	intf := pcapgo.DefaultNgInterface
	intf.LinkType = linkType
	return p.NewNgWriterInterface(w, intf, pcapgo.DefaultNgWriterOptions)
}

// AddInterface is NgWriter.AddInterface (ngwrite.go:237-298): it returns the new interface's id.
func (w *NgWriter) AddInterface(intf pcapgo.NgInterface) (int, error) {
	strs, d := ngStrs(intf.Name, intf.Comment, intf.Description, intf.Filter, intf.OS)
	c := C.gpd_pcapng_iface{name: d[0], comment: d[1], description: d[2], filter: d[3], os: d[4],
		ts_offset: C.uint64_t(intf.TimestampOffset), linktype: C.uint32_t(intf.LinkType),
		snaplen: C.uint32_t(intf.SnapLength), ts_resolution: C.uint32_t(intf.TimestampResolution)}
	block, err := ngBlock("gpd_pcapng_interface_block", func(out *C.uint8_t, cap C.uint64_t, n *C.uint64_t) C.int {
		return C.gpd_pcapng_interface_block(&c, (*C.uint8_t)(bytesPtr(strs)), C.uint64_t(len(strs)), out, cap, n)
	})
	if err != nil {
		return 0, err
	}
	id := int(w.intf)
	w.intf++
	_, err = w.w.Write(block)
	return id, err
}

// WriteInterfaceStats is NgWriter.WriteInterfaceStats (ngwrite.go:301-353).
func (w *NgWriter) WriteInterfaceStats(intf int, stats pcapgo.NgInterfaceStatistics) error {
	has := func(t time.Time) C.uint32_t {
		if t.IsZero() {
			return 0
		}
		return 1
	}
	c := C.gpd_pcapng_stats{last_update: C.uint64_t(stats.LastUpdate.UnixNano()), start_time: C.uint64_t(stats.StartTime.UnixNano()),
		end_time: C.uint64_t(stats.EndTime.UnixNano()), packets_received: C.uint64_t(stats.PacketsReceived),
		packets_dropped: C.uint64_t(stats.PacketsDropped), has_last_update: has(stats.LastUpdate),
		has_start_time: has(stats.StartTime), has_end_time: has(stats.EndTime)}
	block, err := ngBlock("gpd_pcapng_stats_block", func(out *C.uint8_t, cap C.uint64_t, n *C.uint64_t) C.int {
		return C.gpd_pcapng_stats_block(C.int64_t(intf), C.uint32_t(w.intf), &c, out, cap, n)
	})
	if err != nil {
		return err
	}
	_, err = w.w.Write(block)
	return err
}

// WriteBatch is the loop
//
//	for i := range ci { if keep[i] { err = w.WritePacket(ci[i], b.Packet(i)) } }
//
// run on the device: it returns the records written.  Like the loop it stops at the first kept
// packet whose InterfaceIndex was not added or whose CaptureLength > Length, after writing the
// records before it.  The Timestamp is written as it is (ngwrite.go:371).  keep may be nil.
func (w *NgWriter) WriteBatch(b *PacketBatch, ci []gopacket.CaptureInfo, keep []bool) (int, error) {
	n := len(b.Offset)
	if n == 0 {
		return 0, nil
	}
	if len(ci) < n || (keep != nil && len(keep) < n) {
		return 0, errors.New("gpdecode: WriteBatch needs a CaptureInfo (and keep flag) per packet")
	}
	p := w.p
	if err := p.configure(); err != nil {
		return 0, err
	}
	done, err := p.onDevice()
	if err != nil {
		return 0, err
	}
	defer done()
	in, dkeep, free, err := p.upload(b, keep)
	defer free()
	if err != nil {
		return 0, err
	}
	ts, wl, ifx := make([]uint64, n), make([]uint32, n), make([]uint32, n)
	for i := range ts {
		ts[i], wl[i], ifx[i] = uint64(ci[i].Timestamp.UnixNano()), uint32(ci[i].Length), uint32(ci[i].InterfaceIndex)
	}
	var dev [3]devBuf
	for j, c := range []struct {
		src   unsafe.Pointer
		bytes int
	}{{unsafe.Pointer(&ts[0]), 8 * n}, {unsafe.Pointer(&wl[0]), 4 * n}, {unsafe.Pointer(&ifx[0]), 4 * n}} {
		if dev[j], err = devAlloc(c.bytes); err != nil {
			return 0, err
		}
		defer dev[j].free()
		if err := toDev(dev[j], c.src, c.bytes); err != nil {
			return 0, err
		}
	}
	call := func(out unsafe.Pointer, cap uint64) (C.int, uint64, uint64) {
		var nw, nb, bad C.uint64_t
		var why C.uint32_t
		rc := C.gpd_pcapng_write(p.ctx, &in, (*C.uint64_t)(dev[0].p), (*C.uint32_t)(dev[1].p), (*C.uint32_t)(dev[2].p),
			C.uint32_t(w.intf), (*C.uint8_t)(dkeep.p), nil, 0, (*C.uint8_t)(out), C.uint64_t(cap), &nw, &nb, &bad, &why, nil)
		return rc, uint64(nw), uint64(nb)
	}
	rc, _, need := call(nil, 0) // the sizing call
	if rc != C.GPD_OK && rc != C.GPD_ERR_PCAP {
		return 0, lastError("gpd_pcapng_write", rc)
	}
	dout, err := devAlloc(int(need))
	if err != nil {
		return 0, err
	}
	defer dout.free()
	rc, nw, nb := call(dout.p, need)
	if rc != C.GPD_OK && rc != C.GPD_ERR_PCAP {
		return 0, lastError("gpd_pcapng_write", rc)
	}
	werr := lastError("gpd_pcapng_write", rc) // the rejected packet's text; read before any other call
	if nb > 0 {
		host := make([]byte, nb)
		if e := C.hipMemcpy(unsafe.Pointer(&host[0]), dout.p, C.size_t(nb), C.hipMemcpyDeviceToHost); e != C.hipSuccess {
			return 0, errors.New(C.GoString(C.hipGetErrorString(e)))
		}
		if _, err := w.w.Write(host); err != nil {
			return int(nw), err
		}
	}
	runtime.KeepAlive(b)
	if rc == C.GPD_ERR_PCAP {
		return int(nw), werr
	}
	return int(nw), nil
}
