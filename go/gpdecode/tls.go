package gpdecode

// The TLS record decode (include/gpd_tls.h) from Go: layers.TLS for every packet of a batch whose
// decode stopped at LayerTypeTLS, and for reassembled byte streams, walked on the device and handed
// back as layers.TLS values.  Not compiled here (no Go toolchain); tests/test_tls_gpu.py drives the
// same C entry points through ctypes on the GPU.

/*
#cgo CFLAGS: -I${SRCDIR}/../../include -I/opt/rocm/include -D__HIP_PLATFORM_AMD__
#cgo LDFLAGS: -L/opt/rocm/lib -lamdhip64
#include <hip/hip_runtime_api.h>
#include "gpd.h"
#include "gpd_tls.h"
*/
import "C"

import (
	"errors"
	"fmt"
	"runtime"
	"unsafe"

	"github.com/google/gopacket/layers"
)

// TLSMessage is one message: the packet (or range) it came from, the layer as DecodeFromBytes
// leaves it and the error that call returned.  A caller with &tls in its DecodingLayerParser
// composes decoded + [LayerTypeTLS] when Err is nil, and returns Err as DecodeLayers would
// otherwise.  ErrOff is where a stream consumer takes up again: data[ErrOff:] is carried into the
// next batch's bytes of the connection.
type TLSMessage struct {
	Packet    int
	TLS       layers.TLS
	Err       error
	Truncated bool
	ErrOff    int
}

// tlsErrorText is the reference's error text of a verdict (layers/tls.go:133,147,154,
// tls_cipherspec.go:45, tls_alert.go:82, tls_appdata.go:29).
var tlsErrorText = [...]string{
	C.GPD_TLS_E_TOO_SHORT:       "TLS record too short",
	C.GPD_TLS_E_UNKNOWN_TYPE:    "Unknown TLS record type",
	C.GPD_TLS_E_LENGTH_MISMATCH: "TLS packet length mismatch",
	C.GPD_TLS_E_CCS_LENGTH:      "TLS Change Cipher Spec record incorrect length",
	C.GPD_TLS_E_ALERT_SHORT:     "TLS Alert packet too short",
	C.GPD_TLS_E_APPDATA_LENGTH:  "TLS Application Data length mismatch",
}

func tlsError(m *C.gpd_tls_msg) error {
	v := int(m.verdict)
	if v == C.GPD_TLS_OK {
		return nil
	}
	if v >= len(tlsErrorText) || tlsErrorText[v] == "" {
		return fmt.Errorf("gpd: unknown TLS verdict %d", v)
	}
	return errors.New(tlsErrorText[v])
}

// tlsBuild fills msg.TLS from one message record and its record entries (recs begins at the
// message's first).  Every entry carries its index in its own list, so the four lists are
// allocated once and filled without a scan.
func tlsBuild(msg *TLSMessage, m *C.gpd_tls_msg, recs []C.gpd_tls_rec, data []byte) {
	msg.Err = tlsError(m)
	msg.Truncated = m.truncated != 0
	msg.ErrOff = int(m.err_off)
	t := &msg.TLS
	t.BaseLayer = layers.BaseLayer{Contents: data[int(m.contents_off):]}
	if m.n_ccs > 0 {
		t.ChangeCipherSpec = make([]layers.TLSChangeCipherSpecRecord, int(m.n_ccs))
	}
	if m.n_handshake > 0 {
		t.Handshake = make([]layers.TLSHandshakeRecord, int(m.n_handshake))
	}
	if m.n_appdata > 0 {
		t.AppData = make([]layers.TLSAppDataRecord, int(m.n_appdata))
	}
	if m.n_alert > 0 {
		t.Alert = make([]layers.TLSAlertRecord, int(m.n_alert))
	}
	n := int(m.n_ccs) + int(m.n_handshake) + int(m.n_appdata) + int(m.n_alert)
	for k := 0; k < n; k++ {
		r := &recs[k]
		h := layers.TLSRecordHeader{ContentType: layers.TLSType(r.content_type), Version: layers.TLSVersion(r.version),
			Length: uint16(r.length)}
		body := data[int(r.off)+5 : int(r.off)+5+int(r.length)]
		i := int(r.index_in_kind)
		switch h.ContentType {
		case layers.TLSChangeCipherSpec:
			t.ChangeCipherSpec[i] = layers.TLSChangeCipherSpecRecord{TLSRecordHeader: h, Message: layers.TLSchangeCipherSpec(r.a)}
		case layers.TLSAlert:
			a := layers.TLSAlertRecord{TLSRecordHeader: h, Level: layers.TLSAlertLevel(r.a), Description: layers.TLSAlertDescr(r.b)}
			if r.flags&C.GPD_TLS_REC_ENCRYPTED != 0 {
				a.EncryptedMsg = body
			}
			t.Alert[i] = a
		case layers.TLSHandshake:
			t.Handshake[i] = layers.TLSHandshakeRecord{TLSRecordHeader: h}
		case layers.TLSApplicationData:
			t.AppData[i] = layers.TLSAppDataRecord{TLSRecordHeader: h, Payload: body}
		}
	}
}

// DecodeTLSBytes is (*layers.TLS).DecodeFromBytes for one message in host memory through the host
// walker (gpd_tls_decode_host, no device, no budget): what a deferred message goes through.
func DecodeTLSBytes(data []byte) (*TLSMessage, error) {
	var m C.gpd_tls_msg
	var cnt C.gpd_tls_counts
	var p *C.uint8_t
	if len(data) > 0 {
		p = (*C.uint8_t)(unsafe.Pointer(&data[0]))
	}
	C.gpd_tls_decode_host(p, C.uint32_t(len(data)), 0, &m, nil, 0, &cnt) // the sizing call
	recs := make([]C.gpd_tls_rec, int(cnt.records)+1)
	if rc := C.gpd_tls_decode_host(p, C.uint32_t(len(data)), 0, &m, &recs[0], cnt.records, &cnt); rc != C.GPD_OK {
		return nil, lastError("gpd_tls_decode_host", rc)
	}
	out := &TLSMessage{}
	tlsBuild(out, &m, recs, data)
	runtime.KeepAlive(data)
	return out, nil
}

func tlsConfig(maxRecords uint32) C.gpd_tls_config {
	cfg := C.gpd_tls_config{max_records: C.GPD_TLS_MAX_RECORDS_DEFAULT}
	if maxRecords != 0 {
		cfg.max_records = C.uint32_t(maxRecords)
	}
	return cfg
}

// tlsCollect runs `call` as the sizing call, allocates the two arrays, runs it again and builds
// the messages; dataOf returns the bytes of message m.
func tlsCollect(who string, call func(out *C.gpd_tls_out, cnt *C.gpd_tls_counts) C.int,
	dataOf func(m *C.gpd_tls_msg) []byte) ([]TLSMessage, error) {
	var cnt C.gpd_tls_counts
	var out C.gpd_tls_out
	rc := call(&out, &cnt) // the sizing call
	if rc == C.GPD_OK {
		return nil, nil // no message
	}
	if cnt.msgs == 0 {
		return nil, lastError(who, rc)
	}
	nm, nr := int(cnt.msgs), int(cnt.records)
	dm, err := devAlloc(nm * C.sizeof_gpd_tls_msg)
	if err != nil {
		return nil, err
	}
	defer dm.free()
	dr, err := devAlloc(nr*C.sizeof_gpd_tls_rec + 16)
	if err != nil {
		return nil, err
	}
	defer dr.free()
	out = C.gpd_tls_out{msgs: (*C.gpd_tls_msg)(dm.p), cap_msgs: cnt.msgs, recs: (*C.gpd_tls_rec)(dr.p), cap_recs: cnt.records}
	if rc := call(&out, &cnt); rc != C.GPD_OK {
		return nil, lastError(who, rc)
	}
	msgs := make([]C.gpd_tls_msg, nm)
	recs := make([]C.gpd_tls_rec, nr+1)
	if err := fromDev(unsafe.Pointer(&msgs[0]), dm, nm*C.sizeof_gpd_tls_msg); err != nil {
		return nil, err
	}
	if nr > 0 {
		if err := fromDev(unsafe.Pointer(&recs[0]), dr, nr*C.sizeof_gpd_tls_rec); err != nil {
			return nil, err
		}
	}
	res := make([]TLSMessage, nm)
	for j := range msgs {
		m := &msgs[j]
		data := dataOf(m)
		if m.verdict == C.GPD_TLS_DEFERRED {
			h, err := DecodeTLSBytes(data)
			if err != nil {
				return nil, err
			}
			res[j] = *h
		} else {
			tlsBuild(&res[j], m, recs[int(m.first_record):], data)
		}
		res[j].Packet = int(m.packet)
	}
	return res, nil
}

// DecodeTLS decodes the batch on the device and then every packet whose decode stopped at
// LayerTypeTLS as (*layers.TLS).DecodeFromBytes does, in packet order.  maxRecords is the budget
// of one message on the device (0: the default, 1024); a message over it is decoded by the host
// walker, so the result is the reference's for every candidate.
//
//	msgs, _ := p.DecodeTLS(&b, 0)
//	for _, m := range msgs {
//	    if m.Err == nil { handle(m.Packet, &m.TLS) }     // decoded + [LayerTypeTLS]
//	}
func (p *BatchDecodingLayerParser) DecodeTLS(b *PacketBatch, maxRecords uint32) ([]TLSMessage, error) {
	n := len(b.Offset)
	if n == 0 || len(b.Data) == 0 {
		return nil, nil
	}
	if err := p.configure(); err != nil {
		return nil, err
	}
	done, err := p.onDevice()
	if err != nil {
		return nil, err
	}
	defer done()
	// data, offset, caplen, status, layers, hdr_off
	sizes := []int{(len(b.Data)+15)&^15 + 64, 4 * n, 4 * n, 4 * n, 8 * n, 4 * n}
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
	cfg := tlsConfig(maxRecords)
	out, err := tlsCollect("gpd_tls_decode",
		func(o *C.gpd_tls_out, cnt *C.gpd_tls_counts) C.int {
			return C.gpd_tls_decode(p.ctx, &in, &res, &cfg, o, cnt, nil)
		},
		func(m *C.gpd_tls_msg) []byte {
			at := int(b.Offset[m.packet]) + int(m.data_off)
			return b.Data[at : at+int(m.data_len)]
		})
	runtime.KeepAlive(b)
	return out, err
}

// DecodeTLSRanges runs the same decode over byte ranges of one buffer, e.g. the bytes tcpassembly
// handed each Stream: range k is data[off[k] : off[k]+length[k]], one message each (Packet is k).
// The buffer and the ranges are copied to the device; a caller whose streams already lie in
// device memory (gpd_tcp_assemble) passes them to gpd_tls_decode_ranges directly.
func (p *BatchDecodingLayerParser) DecodeTLSRanges(data []byte, off []uint64, length []uint32, maxRecords uint32) ([]TLSMessage, error) {
	n := len(off)
	if n == 0 {
		return nil, nil
	}
	if len(length) != n {
		return nil, errors.New("gpd: DecodeTLSRanges needs one length for every offset")
	}
	if err := p.configure(); err != nil {
		return nil, err
	}
	done, err := p.onDevice()
	if err != nil {
		return nil, err
	}
	defer done()
	sizes := []int{len(data) + 16, 8 * n, 4 * n}
	bufs := make([]devBuf, len(sizes))
	for k, s := range sizes {
		d, err := devAlloc(s)
		if err != nil {
			return nil, err
		}
		bufs[k] = d
		defer d.free()
	}
	if len(data) > 0 {
		if err := toDev(bufs[0], unsafe.Pointer(&data[0]), len(data)); err != nil {
			return nil, err
		}
	}
	if err := toDev(bufs[1], unsafe.Pointer(&off[0]), 8*n); err != nil {
		return nil, err
	}
	if err := toDev(bufs[2], unsafe.Pointer(&length[0]), 4*n); err != nil {
		return nil, err
	}
	rg := C.gpd_tls_ranges{bytes: (*C.uint8_t)(bufs[0].p), nbytes: C.uint64_t(len(data)),
		off: (*C.uint64_t)(bufs[1].p), len: (*C.uint32_t)(bufs[2].p), n: C.uint64_t(n)}
	cfg := tlsConfig(maxRecords)
	out, err := tlsCollect("gpd_tls_decode_ranges",
		func(o *C.gpd_tls_out, cnt *C.gpd_tls_counts) C.int {
			return C.gpd_tls_decode_ranges(p.ctx, &rg, &cfg, o, cnt, nil)
		},
		func(m *C.gpd_tls_msg) []byte {
			at := int(off[m.packet])
			return data[at : at+int(m.data_len)]
		})
	runtime.KeepAlive(data)
	return out, err
}
