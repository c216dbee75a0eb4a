package gpdecode

// The DHCP message decode (include/gpd_dhcp.h) from Go: layers.DHCPv4 and layers.DHCPv6 for every
// packet of a batch whose decode stopped at LayerTypeDHCPv4 or LayerTypeDHCPv6, walked on the
// device and handed back as layer values.  Not compiled here (no Go toolchain);
// tests/test_dhcp_gpu.py drives the same C entry points through ctypes on the GPU.

/*
#cgo CFLAGS: -I${SRCDIR}/../../include -I/opt/rocm/include -D__HIP_PLATFORM_AMD__
#cgo LDFLAGS: -L/opt/rocm/lib -lamdhip64
#include <hip/hip_runtime_api.h>
#include "gpd.h"
#include "gpd_dhcp.h"
*/
import "C"

import (
	"errors"
	"fmt"
	"net"
	"runtime"
	"unsafe"

	"github.com/google/gopacket/layers"
)

// DHCPMessage is one message: the packet it came from, the layer as DecodeFromBytes leaves it
// (V4 when Version is 4, V6 when it is 6) and the error that call returned.  A caller with
// &dhcp4 / &dhcp6 in its DecodingLayerParser composes decoded + [LayerTypeDHCPv4] or
// decoded + [LayerTypeDHCPv6] when Err is nil, and returns Err as DecodeLayers would otherwise.
// HWPastData: a HardwareLen below 228 passes the message, and ClientHWAddr is clipped to it
// (GPD_DHCP_HW_PAST_DATA; the reference slices by capacity there).  A HardwareLen from 228 up makes
// the reference panic (28+HardwareLen wraps in uint8): Err is then what DecodeLayers returns.
type DHCPMessage struct {
	Packet     int
	Version    int
	V4         layers.DHCPv4
	V6         layers.DHCPv6
	Err        error
	Truncated  bool
	ErrOff     int
	HWPastData bool
}

// dhcpError is the reference's error of a verdict: the three DHCPv4Error constants by identity
// (dhcpv4.go:588-595), the formatted ones by text (dhcpv4.go:129, dhcpv6.go:92,102,
// dhcpv6_options.go:612,617).
func dhcpError(m *C.gpd_dhcp_msg) error {
	switch int(m.verdict) {
	case C.GPD_DHCP_OK:
		return nil
	case C.GPD_DHCP_E_V4_TOO_SHORT:
		return fmt.Errorf("DHCPv4 length %d too short", int(m.err_arg))
	case C.GPD_DHCP_E_V4_BAD_MAGIC:
		return layers.InvalidMagicCookie
	case C.GPD_DHCP_E_V4_OPT_NO_DATA, C.GPD_DHCP_E_V4_OPT_EMPTY:
		return layers.DecOptionNotEnoughData
	case C.GPD_DHCP_E_V4_OPT_MALFORMED:
		return layers.DecOptionMalformed
	case C.GPD_DHCP_E_V4_HW_PANIC: // what DecodeLayers makes of the panic at dhcpv4.go:143 (parser.go:328-332)
		return fmt.Errorf("panic: runtime error: slice bounds out of range [28:%d]", int(m.err_arg))
	case C.GPD_DHCP_E_V6_TOO_SHORT:
		return fmt.Errorf("DHCPv6 length %d too short", int(m.err_arg))
	case C.GPD_DHCP_E_V6_RELAY_SHORT:
		return fmt.Errorf("DHCPv6 length %d too short for message type %d", int(m.err_arg), int(m.op))
	case C.GPD_DHCP_E_V6_OPT_NO_DATA:
		return errors.New("not enough data to decode")
	case C.GPD_DHCP_E_V6_OPT_SIZE:
		return fmt.Errorf("dhcpv6 option size < length %d", int(m.err_arg))
	}
	return fmt.Errorf("gpd: unknown DHCP verdict %d", int(m.verdict))
}

// dhcpBuild fills msg from one message record and its option entries (opts begins at the
// message's first).  Every slice is a slice of data, as in the reference.
func dhcpBuild(msg *DHCPMessage, m *C.gpd_dhcp_msg, opts []C.gpd_dhcp_opt, data []byte) {
	msg.Version = int(m.version)
	msg.Err = dhcpError(m)
	msg.Truncated = m.truncated != 0
	msg.ErrOff = int(m.err_off)
	msg.HWPastData = m.mflags&C.GPD_DHCP_HW_PAST_DATA != 0
	n := int(m.n_opts)
	if msg.Version == 4 {
		d := &msg.V4
		if m.verdict != C.GPD_DHCP_E_V4_TOO_SHORT {
			d.Operation, d.HardwareType = layers.DHCPOp(m.op), layers.LinkType(m.htype)
			d.HardwareLen, d.HardwareOpts = uint8(m.hlen), uint8(m.hops)
			d.Xid, d.Secs, d.Flags = uint32(m.xid), uint16(m.secs), uint16(m.flags)
			d.ClientIP, d.YourClientIP = net.IP(data[12:16]), net.IP(data[16:20])
			d.NextServerIP, d.RelayAgentIP = net.IP(data[20:24]), net.IP(data[24:28])
			if m.verdict != C.GPD_DHCP_E_V4_HW_PANIC { // (the panic at :143 comes before these three)
				end := 28 + int(m.hlen)
				if end > len(data) {
					end = len(data)
				}
				d.ClientHWAddr = net.HardwareAddr(data[28:end])
				d.ServerName, d.File = data[44:108], data[108:236]
			}
		}
		if n > 0 {
			d.Options = make(layers.DHCPOptions, n)
		}
		for k := 0; k < n; k++ {
			o := &opts[k]
			d.Options[k] = layers.DHCPOption{Type: layers.DHCPOpt(o.code), Length: uint8(o.length)}
			if o.code != C.GPD_DHCP_V4_PAD {
				d.Options[k].Data = data[int(o.off)+2 : int(o.off)+2+int(o.length)]
			}
		}
		if m.mflags&C.GPD_DHCP_CONTENTS != 0 {
			d.Contents = data
		}
		return
	}
	d := &msg.V6
	if m.mflags&C.GPD_DHCP_CONTENTS != 0 {
		d.BaseLayer = layers.BaseLayer{Contents: data}
		d.MsgType = layers.DHCPv6MsgType(m.op)
	}
	if m.mflags&C.GPD_DHCP_RELAY != 0 {
		d.HopCount, d.LinkAddr, d.PeerAddr = uint8(m.hops), net.IP(data[2:18]), net.IP(data[18:34])
	} else if len(data) >= 4 && m.verdict != C.GPD_DHCP_E_V6_RELAY_SHORT {
		d.TransactionID = data[1:4]
	}
	if n > 0 {
		d.Options = make(layers.DHCPv6Options, n)
	}
	for k := 0; k < n; k++ {
		o := &opts[k]
		d.Options[k] = layers.DHCPv6Option{Code: layers.DHCPv6Opt(o.code), Length: uint16(o.length),
			Data: data[int(o.off)+4 : int(o.off)+4+int(o.length)]}
	}
}

// DecodeDHCPBytes is (*layers.DHCPv4).DecodeFromBytes (version 4) or
// (*layers.DHCPv6).DecodeFromBytes (version 6) for one message in host memory through the host
// walker (gpd_dhcp_decode_host, no device, no budget): what a deferred message goes through.
func DecodeDHCPBytes(version int, data []byte) (*DHCPMessage, error) {
	var m C.gpd_dhcp_msg
	var cnt C.gpd_dhcp_counts
	var p *C.uint8_t
	if len(data) > 0 {
		p = (*C.uint8_t)(unsafe.Pointer(&data[0]))
	}
	v := C.uint32_t(version)
	C.gpd_dhcp_decode_host(v, p, C.uint32_t(len(data)), 0, &m, nil, 0, &cnt) // the sizing call
	opts := make([]C.gpd_dhcp_opt, int(cnt.options)+1)
	if rc := C.gpd_dhcp_decode_host(v, p, C.uint32_t(len(data)), 0, &m, &opts[0], cnt.options, &cnt); rc != C.GPD_OK {
		return nil, lastError("gpd_dhcp_decode_host", rc)
	}
	out := &DHCPMessage{}
	dhcpBuild(out, &m, opts, data)
	runtime.KeepAlive(data)
	return out, nil
}

// DecodeDHCP decodes the batch on the device and then every packet whose decode stopped at
// LayerTypeDHCPv4 or LayerTypeDHCPv6 as the layer's DecodeFromBytes does, in packet order.
// maxOptions is the budget of one message on the device (0: the default, 2048); a message over it
// is decoded by the host walker, so the result is the reference's for every candidate.
//
//	msgs, _ := p.DecodeDHCP(&b, 0)
//	for _, m := range msgs {
//	    if m.Err == nil && m.Version == 4 { lease(m.Packet, &m.V4) }   // decoded + [LayerTypeDHCPv4]
//	}
func (p *BatchDecodingLayerParser) DecodeDHCP(b *PacketBatch, maxOptions uint32) ([]DHCPMessage, error) {
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
	cfg := C.gpd_dhcp_config{max_options: C.GPD_DHCP_MAX_OPTIONS_DEFAULT}
	if maxOptions != 0 {
		cfg.max_options = C.uint32_t(maxOptions)
	}
	var cnt C.gpd_dhcp_counts
	var out C.gpd_dhcp_out
	rc := C.gpd_dhcp_decode(p.ctx, &in, &res, &cfg, &out, &cnt, nil) // the sizing call
	if rc == C.GPD_OK {
		return nil, nil // no message
	}
	if cnt.msgs == 0 {
		return nil, lastError("gpd_dhcp_decode", rc)
	}
	nm, no := int(cnt.msgs), int(cnt.options)
	dm, err := devAlloc(nm * C.sizeof_gpd_dhcp_msg)
	if err != nil {
		return nil, err
	}
	defer dm.free()
	do, err := devAlloc(no*C.sizeof_gpd_dhcp_opt + 16)
	if err != nil {
		return nil, err
	}
	defer do.free()
	out = C.gpd_dhcp_out{msgs: (*C.gpd_dhcp_msg)(dm.p), cap_msgs: cnt.msgs, opts: (*C.gpd_dhcp_opt)(do.p), cap_opts: cnt.options}
	if rc := C.gpd_dhcp_decode(p.ctx, &in, &res, &cfg, &out, &cnt, nil); rc != C.GPD_OK {
		return nil, lastError("gpd_dhcp_decode", rc)
	}
	msgs := make([]C.gpd_dhcp_msg, nm)
	opts := make([]C.gpd_dhcp_opt, no+1)
	if err := fromDev(unsafe.Pointer(&msgs[0]), dm, nm*C.sizeof_gpd_dhcp_msg); err != nil {
		return nil, err
	}
	if no > 0 {
		if err := fromDev(unsafe.Pointer(&opts[0]), do, no*C.sizeof_gpd_dhcp_opt); err != nil {
			return nil, err
		}
	}
	ret := make([]DHCPMessage, nm)
	for j := range msgs {
		m := &msgs[j]
		at := int(b.Offset[m.packet]) + int(m.data_off)
		data := b.Data[at : at+int(m.data_len)]
		if m.verdict == C.GPD_DHCP_DEFERRED {
			h, err := DecodeDHCPBytes(int(m.version), data)
			if err != nil {
				return nil, err
			}
			ret[j] = *h
		} else {
			dhcpBuild(&ret[j], m, opts[int(m.first_opt):], data)
		}
		ret[j].Packet = int(m.packet)
	}
	runtime.KeepAlive(b)
	return ret, nil
}
