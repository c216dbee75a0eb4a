"""Generate tests/golden/tcpfsm_vectors.json (the TCPSimpleFSM fixtures of the connection tracker).

Run where a checkout of the reference (google/gopacket) is at hand; it is read as text:
    python tests/golden/make_tcpfsm_vectors.py <path to the reference>

What it writes is DATA: per step of the reference's FSM tests the four flags CheckState reads, the
two ports (the tests derive the direction from them: the first packet's source port is the
client's), the payload length, and what the test asserts after the step — CheckState's result
(reassembly/tcpcheck_test.go: TestCheckFSM, TestCheckFSMmissingSYNACK, and TestCheckFSMmissingSYN
once per option value) or the running count of accepted packets
(reassembly/tcpassembly_test.go: TestFSMnormalFlow, TestFSMearlyRST, TestFSMestablishedThenRST,
TestFSMmissingSYNACK, which drive the FSM from Stream.Accept with the zero options).
"""
import json
import os
import re
import sys

OUT = os.path.dirname(os.path.abspath(__file__))

CHECK = "reassembly/tcpcheck_test.go"
ASM = "reassembly/tcpassembly_test.go"
TESTS = [(CHECK, "TestCheckFSM", "expected"), (CHECK, "TestCheckFSMmissingSYNACK", "expected"),
         (CHECK, "TestCheckFSMmissingSYN", "expected"), (ASM, "TestFSMnormalFlow", "nb"),
         (ASM, "TestFSMearlyRST", "nb"), (ASM, "TestFSMestablishedThenRST", "nb"),
         (ASM, "TestFSMmissingSYNACK", "nb")]


def body_of(src, name):
    """The text of `func name(` up to the next top-level func; returns (text, first line)."""
    i = src.index(f"func {name}(t *testing.T)")
    j = src.find("\nfunc ", i + 1)
    return src[i:j if j > 0 else len(src)], src[:i].count("\n") + 1


def steps_of(text, kind):
    out = []
    for part in text.split("tcp: layers.TCP{")[1:]:
        tcp, rest = part.split("ci: gopacket.CaptureInfo{", 1)
        flag = lambda f: re.search(rf"\b{f}:\s*true", tcp) is not None
        num = lambda f: int(re.search(rf"\b{f}:\s*(\d+)", tcp).group(1))
        pay = re.search(r"Payload:\s*\[\]byte\{([^}]*)\}", tcp)
        step = {"syn": flag("SYN"), "ack": flag("ACK"), "fin": flag("FIN"), "rst": flag("RST"),
                "sport": num("SrcPort"), "dport": num("DstPort"),
                "payload_len": len(re.findall(r"\d+", pay.group(1))) if pay else 0}
        want = re.search(rf"\b{kind}:\s*(\w+)", rest).group(1)
        step[kind] = want if want == "val" else (want == "true" if kind == "expected" else int(want))
        out.append(step)
    return out


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = sys.argv[1]
    seqs = []
    for path, name, kind in TESTS:
        text, line = body_of(open(os.path.join(ref, path)).read(), name)
        steps = steps_of(text, kind)
        per_option = any(s[kind] == "val" for s in steps)  # `for _, val := range []bool{false, true}`
        for val in ((False, True) if per_option else (False,)):
            mine = [dict(s, **{kind: val if s[kind] == "val" else s[kind]}) for s in steps]
            seqs.append({"test": name, "source": f"{path}:{line}", "support_missing_establishment": val,
                         "asserts": kind, "steps": mine})
    doc = {"fsm": "reassembly/tcpcheck.go:119-246", "sequences": seqs}
    with open(os.path.join(OUT, "tcpfsm_vectors.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
