package gpdecode

// The DNS message decode (include/gpd_dns.h) from Go: layers.DNS for every packet of a batch
// whose decode stopped at LayerTypeDNS, validated and decompressed on the device and handed back
// as layers.DNS values.  Not compiled here (no Go toolchain); tests/test_dns_gpu.py drives the
// same C entry points through ctypes on the GPU.

/*
#cgo CFLAGS: -I${SRCDIR}/../../include -I/opt/rocm/include -D__HIP_PLATFORM_AMD__
#cgo LDFLAGS: -L/opt/rocm/lib -lamdhip64
#include <hip/hip_runtime_api.h>
#include "gpd.h"
#include "gpd_dns.h"
*/
import "C"

import (
	"encoding/binary"
	"errors"
	"fmt"
	"runtime"
	"unsafe"

	"github.com/google/gopacket/layers"
)

// DNSMessage is one candidate: the packet it came from, the layer as DecodeFromBytes leaves it
// and the error that call returned.  A caller with &dns in its DecodingLayerParser composes
// decoded + [LayerTypeDNS] when Err is nil, and returns Err as DecodeLayers would otherwise.
type DNSMessage struct {
	Packet    int
	DNS       layers.DNS
	Err       error
	Truncated bool
}

// dnsErrorText is the reference's error text of a verdict (layers/dns.go:1089-1107 and the
// inline errors); the verbs take err_arg0 and err_arg1.
var dnsErrorText = [...]string{
	C.GPD_DNS_E_TOO_SHORT:          "DNS packet too short",
	C.GPD_DNS_E_MAX_RECURSION:      "max DNS recursion level hit",
	C.GPD_DNS_E_NAME_OFFSET_HIGH:   "dns name offset too high",
	C.GPD_DNS_E_NAME_OFFSET_NEG:    "dns name offset is negative",
	C.GPD_DNS_E_NAME_TOO_LONG:      "dns name is too long",
	C.GPD_DNS_E_NAME_INVALID_INDEX: "dns name uncomputable: invalid index",
	C.GPD_DNS_E_POINTER_HIGH:       "dns offset pointer too high",
	C.GPD_DNS_E_INDEX_RANGE:        "dns index walked out of range",
	C.GPD_DNS_E_NAME_NO_DATA:       "no dns data found for name",
	C.GPD_DNS_E_LABEL_40:           "qname '0x40' - RFC 2673 unsupported yet (data=%x index=%d)",
	C.GPD_DNS_E_LABEL_80:           "qname '0x80' unsupported yet (data=%x index=%d)",
	C.GPD_DNS_E_QUESTION_SMALL:     "DNS question too small",
	C.GPD_DNS_E_RECORD_SMALL:       "DNS record too small",
	C.GPD_DNS_E_RECORD_LENGTH:      "resource record length exceeds data",
	C.GPD_DNS_E_CHAR_STRING:        "Insufficient data for a <character-string>",
	C.GPD_DNS_E_SOA_SMALL:          "SOA too small",
	C.GPD_DNS_E_MX_SMALL:           "MX too small",
	C.GPD_DNS_E_URI_SMALL:          "URI too small",
	C.GPD_DNS_E_SRV_SMALL:          "SRV too small",
	C.GPD_DNS_E_OPT_SHORT:          "DNSOPT record is of length %d, it should be at least length 4",
	C.GPD_DNS_E_OPT_MALFORMED:      "Malformed DNSOPT record.  Length %d < %d",
	C.GPD_DNS_E_OPT_LENGTH:         "Malformed DNSOPT record. The length (%d) field implies a packet larger than the one received",
	C.GPD_DNS_E_BAD_QDCOUNT:        "Invalid query decoding, not the right number of questions",
	C.GPD_DNS_E_BAD_ANCOUNT:        "Invalid query decoding, not the right number of answers",
	C.GPD_DNS_E_BAD_NSCOUNT:        "Invalid query decoding, not the right number of authorities",
	C.GPD_DNS_E_BAD_ARCOUNT:        "Invalid query decoding, not the right number of additionals info",
}

func dnsError(m *C.gpd_dns_msg) error {
	v := int(m.verdict)
	if v == C.GPD_DNS_OK {
		return nil
	}
	if v >= len(dnsErrorText) || dnsErrorText[v] == "" {
		return fmt.Errorf("gpd: unknown DNS verdict %d", v)
	}
	switch v {
	case C.GPD_DNS_E_LABEL_40, C.GPD_DNS_E_LABEL_80, C.GPD_DNS_E_OPT_MALFORMED:
		return fmt.Errorf(dnsErrorText[v], uint32(m.err_arg0), uint32(m.err_arg1))
	case C.GPD_DNS_E_OPT_SHORT, C.GPD_DNS_E_OPT_LENGTH:
		return fmt.Errorf(dnsErrorText[v], uint32(m.err_arg0))
	}
	return errors.New(dnsErrorText[v])
}

// dnsRecord builds one resource record from its entry: the names come from names[], everything
// that is a slice or a fixed read of rr.Data from the message bytes (layers/dns.go:906-993).
func dnsRecord(e *C.gpd_dns_entry, data, names []byte) layers.DNSResourceRecord {
	o := int(e.name_off)
	r := layers.DNSResourceRecord{Name: names[o : o+int(e.name_len)], Type: layers.DNSType(e._type),
		Class: layers.DNSClass(e.klass), TTL: uint32(e.ttl), DataLength: uint16(e.rdlength)}
	off := int(e.rdata_off)
	r.Data = data[off : off+int(e.rdlength)]
	if e.rdlength == 0 { // dns.go:731: decodeRData is skipped
		return r
	}
	o += int(e.name_len)
	n1 := names[o : o+int(e.rname1_len)]
	n2 := names[o+int(e.rname1_len) : o+int(e.rname1_len)+int(e.rname2_len)]
	switch r.Type {
	case layers.DNSTypeA, layers.DNSTypeAAAA:
		r.IP = r.Data
	case layers.DNSTypeTXT, layers.DNSTypeHINFO:
		r.TXT = r.Data
		r.TXTs = make([][]byte, 0, 1)
		for i := 0; i != len(r.Data); i += 1 + int(r.Data[i]) { // (validated on the device)
			r.TXTs = append(r.TXTs, r.Data[i+1:i+1+int(r.Data[i])])
		}
	case layers.DNSTypeNS:
		r.NS = n1
	case layers.DNSTypeCNAME:
		r.CNAME = n1
	case layers.DNSTypePTR:
		r.PTR = n1
	case layers.DNSTypeSOA:
		f := data[int(e.fixed_off):]
		r.SOA = layers.DNSSOA{MName: n1, RName: n2, Serial: binary.BigEndian.Uint32(f[0:4]),
			Refresh: binary.BigEndian.Uint32(f[4:8]), Retry: binary.BigEndian.Uint32(f[8:12]),
			Expire: binary.BigEndian.Uint32(f[12:16]), Minimum: binary.BigEndian.Uint32(f[16:20])}
	case layers.DNSTypeMX:
		r.MX = layers.DNSMX{Preference: binary.BigEndian.Uint16(r.Data[0:2]), Name: n1}
	case layers.DNSTypeURI:
		r.URI = layers.DNSURI{Priority: binary.BigEndian.Uint16(r.Data[0:2]),
			Weight: binary.BigEndian.Uint16(r.Data[2:4]), Target: r.Data[4:]}
	case layers.DNSTypeSRV:
		r.SRV = layers.DNSSRV{Priority: binary.BigEndian.Uint16(r.Data[0:2]),
			Weight: binary.BigEndian.Uint16(r.Data[2:4]), Port: binary.BigEndian.Uint16(r.Data[4:6]), Name: n1}
	case layers.DNSTypeOPT:
		r.OPT = []layers.DNSOPT{}
		for i := 0; i < len(r.Data); {
			l := int(binary.BigEndian.Uint16(r.Data[i+2 : i+4]))
			r.OPT = append(r.OPT, layers.DNSOPT{Code: layers.DNSOptionCode(binary.BigEndian.Uint16(r.Data[i : i+2])),
				Data: r.Data[i+4 : i+4+l]})
			i += 4 + l
		}
	}
	return r
}

// dnsBuild fills msg.DNS from one message record and its entries.
func dnsBuild(msg *DNSMessage, m *C.gpd_dns_msg, ents []C.gpd_dns_entry, data, names []byte) {
	msg.Err = dnsError(m)
	msg.Truncated = m.truncated != 0
	if m.verdict == C.GPD_DNS_E_TOO_SHORT {
		return
	}
	d := &msg.DNS
	f := uint16(m.flags)
	d.BaseLayer = layers.BaseLayer{Contents: data}
	d.ID = uint16(m.id)
	d.QR, d.OpCode = f&0x8000 != 0, layers.DNSOpCode(f>>11&0xF)
	d.AA, d.TC, d.RD, d.RA = f&0x0400 != 0, f&0x0200 != 0, f&0x0100 != 0, f&0x0080 != 0
	d.Z = uint8(f >> 4 & 7)
	d.ResponseCode = layers.DNSResponseCode(m.rcode)
	d.QDCount, d.ANCount, d.NSCount, d.ARCount = uint16(m.qdcount), uint16(m.ancount), uint16(m.nscount), uint16(m.arcount)
	k := 0
	for ; k < int(m.n_q); k++ {
		e := &ents[k]
		d.Questions = append(d.Questions, layers.DNSQuestion{Name: names[int(e.name_off) : int(e.name_off)+int(e.name_len)],
			Type: layers.DNSType(e._type), Class: layers.DNSClass(e.klass)})
	}
	for _, sec := range []struct {
		n   int
		dst *[]layers.DNSResourceRecord
	}{{int(m.n_an), &d.Answers}, {int(m.n_ns), &d.Authorities}, {int(m.n_ar), &d.Additionals}} {
		for j := 0; j < sec.n; j, k = j+1, k+1 {
			*sec.dst = append(*sec.dst, dnsRecord(&ents[k], data, names))
		}
	}
}

// DecodeDNSBytes is (*layers.DNS).DecodeFromBytes for one message in host memory through the host
// walker (gpd_dns_decode_host, no device, no budget): what a deferred message and DNS over a
// reassembled TCP stream go through.
func DecodeDNSBytes(data []byte) (*DNSMessage, error) {
	var m C.gpd_dns_msg
	var cnt C.gpd_dns_counts
	var p *C.uint8_t
	if len(data) > 0 {
		p = (*C.uint8_t)(unsafe.Pointer(&data[0]))
	}
	C.gpd_dns_decode_host(p, C.uint32_t(len(data)), 0, &m, nil, 0, nil, 0, &cnt) // the sizing call
	ents := make([]C.gpd_dns_entry, int(cnt.entries)+1)
	names := make([]byte, int(cnt.name_bytes)+1)
	if rc := C.gpd_dns_decode_host(p, C.uint32_t(len(data)), 0, &m, &ents[0], cnt.entries,
		(*C.uint8_t)(unsafe.Pointer(&names[0])), cnt.name_bytes, &cnt); rc != C.GPD_OK {
		return nil, lastError("gpd_dns_decode_host", rc)
	}
	out := &DNSMessage{}
	dnsBuild(out, &m, ents, data, names)
	runtime.KeepAlive(data)
	return out, nil
}

// DecodeDNS decodes the batch on the device and then every packet whose decode stopped at
// LayerTypeDNS as (*layers.DNS).DecodeFromBytes does, in packet order.  maxWork is the work
// budget of one message on the device (0: the default, 4096); a message over it is decoded by
// the host walker, so the result is the reference's for every candidate.
//
//	msgs, _ := p.DecodeDNS(&b, 0)
//	for _, m := range msgs {
//	    if m.Err == nil { handle(m.Packet, &m.DNS) }     // decoded + [LayerTypeDNS]
//	}
func (p *BatchDecodingLayerParser) DecodeDNS(b *PacketBatch, maxWork uint32) ([]DNSMessage, error) {
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
	cfg := C.gpd_dns_config{max_work: C.GPD_DNS_MAX_WORK_DEFAULT}
	if maxWork != 0 {
		cfg.max_work = C.uint32_t(maxWork)
	}
	var cnt C.gpd_dns_counts
	var out C.gpd_dns_out
	rc := C.gpd_dns_decode(p.ctx, &in, &res, &cfg, &out, &cnt, nil) // the sizing call
	if rc == C.GPD_OK {
		return nil, nil // no candidate
	}
	if cnt.msgs == 0 {
		return nil, lastError("gpd_dns_decode", rc)
	}
	nm, ne, nb := int(cnt.msgs), int(cnt.entries), int(cnt.name_bytes)
	dm, err := devAlloc(nm * C.sizeof_gpd_dns_msg)
	if err != nil {
		return nil, err
	}
	defer dm.free()
	de, err := devAlloc(ne*C.sizeof_gpd_dns_entry + 16)
	if err != nil {
		return nil, err
	}
	defer de.free()
	dn, err := devAlloc(nb + 16)
	if err != nil {
		return nil, err
	}
	defer dn.free()
	out = C.gpd_dns_out{msgs: (*C.gpd_dns_msg)(dm.p), cap_msgs: cnt.msgs, entries: (*C.gpd_dns_entry)(de.p),
		cap_entries: cnt.entries, names: (*C.uint8_t)(dn.p), cap_names: cnt.name_bytes}
	if rc := C.gpd_dns_decode(p.ctx, &in, &res, &cfg, &out, &cnt, nil); rc != C.GPD_OK {
		return nil, lastError("gpd_dns_decode", rc)
	}
	msgs := make([]C.gpd_dns_msg, nm)
	ents := make([]C.gpd_dns_entry, ne+1)
	names := make([]byte, nb+1)
	if err := fromDev(unsafe.Pointer(&msgs[0]), dm, nm*C.sizeof_gpd_dns_msg); err != nil {
		return nil, err
	}
	if ne > 0 {
		if err := fromDev(unsafe.Pointer(&ents[0]), de, ne*C.sizeof_gpd_dns_entry); err != nil {
			return nil, err
		}
	}
	if nb > 0 {
		if err := fromDev(unsafe.Pointer(&names[0]), dn, nb); err != nil {
			return nil, err
		}
	}
	res2 := make([]DNSMessage, nm)
	for j := range msgs {
		m := &msgs[j]
		at := int(b.Offset[m.packet]) + int(m.data_off)
		data := b.Data[at : at+int(m.data_len)]
		if m.verdict == C.GPD_DNS_DEFERRED {
			h, err := DecodeDNSBytes(data)
			if err != nil {
				return nil, err
			}
			res2[j] = *h
		} else {
			dnsBuild(&res2[j], m, ents[int(m.first_entry):], data, names)
		}
		res2[j].Packet = int(m.packet)
	}
	runtime.KeepAlive(b)
	return res2, nil
}
