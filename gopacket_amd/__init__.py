"""gopacket_amd — MI355X-native batched DecodingLayerParser / Flow engine.

The product path is libgpd.so (HIP kernels for gfx950 behind the C-ABI in
include/gpd.h); this package is the host-side mirror of gopacket's parser API
(parser.py), its dispatch tables (layers.py), batch layout (batch.py), result
reading (results.py), input formats (pcap.py, pcapng.py, afpacket.py, synth.py), the pcap and
pcapng writers and batch selection (pcapwrite.py), BPF filtering of a device batch (bpf.py), the flow
table (flows.py), the IPv4 fragment hand-off to ip4defrag (defrag.py) and the TCP segment
hand-off to tcpassembly (tcpassembly.py) and the stream assembly over it (tcpstream.py: the
Reassembly lists per connection, built on the device) and the IPv4 defragmentation over the
fragment hand-off (ip4reasm.py: ip4defrag's datagrams rebuilt on the device; its checker is the
restated defragmenter oracle/ip4defrag_ref.py driven by tests/ip4reasm_ref.py) and the stateful
TCP assembler (tcpasm.py: tcpassembly's Assembler + StreamPool as a device object that keeps
out-of-order data across batches, with FlushOlderThan / FlushAll) and TCP connection tracking
(tcptrack.py: reassembly's bidirectional connection, packet direction and TCPSimpleFSM verdicts,
one state machine per connection kept on the device; its model is tests/tcptrack_ref.py) and flow expiry
(flowexpire.py: idle flow records removed and their slots reused, so that all of these can run
without a table reset; its model is tests/flow_expire_ref.py) and the DNS message decode (dns.py:
layers.DNS for the packets whose decode stopped at LayerTypeDNS, validated and decompressed on the
device; its model is tests/dns_ref.py) and the TLS record decode (tls.py: layers.TLS for the
packets whose decode stopped at LayerTypeTLS and for reassembled streams where they lie; its model
is tests/tls_ref.py) and the DHCP message decode (dhcp.py: layers.DHCPv4 and layers.DHCPv6 for the
packets whose decode stopped at LayerTypeDHCPv4 or LayerTypeDHCPv6; its model is tests/dhcp_ref.py).  (The stream
assembler's restatement tests/tcpassembly_ref.py is the oracle of tcpstream.py.)
"""
from . import layers
from .layers import *  # noqa: F401,F403  LayerType constants, Register*PortLayerType
from .batch import PacketBatch
from .errors import DecodeError, UnsupportedLayerType
from .results import (BatchResult, Endpoint, FastHashes, Flow, FlowFromEndpoints, MaxEndpointSize,
                      NewEndpoint, NewFlow)

__all__ = ["layers", "PacketBatch", "BatchResult", "DecodeError", "UnsupportedLayerType",
           "Endpoint", "Flow", "NewEndpoint", "NewFlow", "FlowFromEndpoints", "FastHashes",
           "MaxEndpointSize", "parser", "pcapng", "pcapwrite", "bpf", "tcpassembly", "tcpstream", "ip4reasm", "tcpasm",
           "tcptrack", "flowexpire", "dns", "tls", "dhcp"]


def __getattr__(name):
    # the parser pulls in libgpd.so; import it lazily so that pure-host helpers
    # (pcap, synth, layers) work in environments that only build.
    # (pcapng, pcapwrite, bpf, tcpassembly, tcpstream, ip4reasm, tcpasm, tcptrack, flowexpire, dns, tls and dhcp bind their entry points onto libgpd.so too)
    if name in ("parser", "pcapng", "pcapwrite", "bpf", "tcpassembly", "tcpstream", "ip4reasm", "tcpasm",
                "tcptrack", "flowexpire", "dns", "tls", "dhcp"):
        import importlib
        return importlib.import_module("." + name, __name__)
    if name in ("NgWriter", "NewNgWriter", "NewNgWriterInterface"):  # the pcapng writer (pcapwrite.py)
        import importlib
        return getattr(importlib.import_module(".pcapwrite", __name__), name)
    raise AttributeError(name)
