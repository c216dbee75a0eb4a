"""TCP connection tracking (include/gpd_tcptrack.h) on the CPU: the model (tests/tcptrack_ref.py)
against the reference's own FSM tests, the ABI and the layouts, the step function and the map
algebra of the kernels (gopacket_amd/csrc/gpd_tcptrack_fsm.h) compiled for the host under the
sanitizers, and the entry points' no-device paths."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import tcptrack_ref as TR
from conftest import ROOT

VEC = json.load(open(os.path.join(ROOT, "tests", "golden", "tcpfsm_vectors.json")))


# ---------------------------------------------------------------- the model against the reference's tests
def vector_packets(seq):
    """(keys, flags) of a golden sequence: one connection, the direction from the ports as the
    reference's test drivers derive it (the first packet's source port is the client's)."""
    keys, flags = [], []
    for s in seq["steps"]:
        keys.append(("a", "b", s["sport"], s["dport"]) if s["sport"] == seq["steps"][0]["sport"]
                    else ("b", "a", s["sport"], s["dport"]))
        flags.append((TR.SYN if s["syn"] else 0) | (TR.ACK if s["ack"] else 0) | (TR.FIN if s["fin"] else 0) |
                     (TR.RST if s["rst"] else 0))
    return keys, flags


def vector_accepts(seq):
    """The accept bit each step of a golden sequence asserts."""
    if seq["asserts"] == "expected":
        return [bool(s["expected"]) for s in seq["steps"]]
    nb = [0] + [s["nb"] for s in seq["steps"]]
    return [b - a == 1 for a, b in zip(nb, nb[1:])]


def test_golden_holds_the_references_fsm_tests():
    names = [s["test"] for s in VEC["sequences"]]
    assert names == ["TestCheckFSM", "TestCheckFSMmissingSYNACK", "TestCheckFSMmissingSYN", "TestCheckFSMmissingSYN",
                     "TestFSMnormalFlow", "TestFSMearlyRST", "TestFSMestablishedThenRST", "TestFSMmissingSYNACK"]
    assert [s["support_missing_establishment"] for s in VEC["sequences"]] == [False, False, False, True] + [False] * 4
    assert [len(s["steps"]) for s in VEC["sequences"]] == [7, 3, 3, 3, 12, 5, 7, 3]


@pytest.mark.parametrize("k", range(8))
def test_model_reproduces_every_golden_sequence(k):
    seq = VEC["sequences"][k]
    keys, flags = vector_packets(seq)
    m = TR.Model(seq["support_missing_establishment"])
    verdict, conn, counts = m.track(keys, flags, list(range(len(keys))))
    assert [bool(v & 1) for v in verdict] == vector_accepts(seq), seq["test"]
    assert [bool(v & 2) for v in verdict] == [key[0] == "b" for key in keys]
    assert (conn == 0).all() and counts == (len(keys), sum(vector_accepts(seq)), len(keys) - sum(vector_accepts(seq)), 1)
    # the same through the FSM alone, as tcpcheck_test.go drives it
    f = TR.TCPSimpleFSM(seq["support_missing_establishment"])
    got = [f.CheckState(bool(fl & TR.SYN), bool(fl & TR.ACK), bool(fl & TR.FIN), bool(fl & TR.RST), key[0] == "b")
           for key, fl in zip(keys, flags)]
    assert got == vector_accepts(seq)
    if seq["test"] == "TestFSMnormalFlow":
        assert f.String() == "Closed" and TR.STATE_NAMES[(int(verdict[-2]) >> 2) & 7] == "LastAck"
    if seq["test"] in ("TestFSMearlyRST", "TestFSMestablishedThenRST"):
        assert f.String() == "Reset"


def test_model_pool_directions():
    m = TR.Model()
    ka, kb, kc = ("a", "b", 1, 2), ("b", "a", 2, 1), ("a", "a", 5, 5)
    v, c, counts = m.track([kb, ka, None, kc, kc], [TR.SYN, TR.SYN | TR.ACK, 0, TR.SYN, TR.ACK], [10, 11, 12, 13, 13])
    assert list(c) == [10, 10, TR.FLOW_NONE, 13, 13] and list(v) == [1 | 4, 1 | 2 | 8, 0xFF, 1 | 4, 0 | 4]
    assert counts == (4, 3, 1, 2)
    st = m.states(16)
    assert st[10] == TR.TCPStateEstablished and st[13] == TR.TCPStateSynSent and st.sum() == 3
    m.forget([10])
    assert m.states(16)[10] == 0 and m.states(16)[13] == 1
    v, c, _ = m.track([ka], [TR.SYN], [11])
    assert list(c) == [10] and list(v) == [1 | 2 | 4 | 0x20]  # still server to client: the records stay


# ---------------------------------------------------------------- the ABI
def test_symbols_exported_and_abi_version_kept():
    from gopacket_amd import _lib
    from gopacket_amd import tcpasm, tcpassembly
    from gopacket_amd import tcptrack as M
    header = open(os.path.join(ROOT, "include", "gpd_tcptrack.h")).read()
    assert list(M.TCPTRACK_EXPORTS) == ["gpd_tcp_tracker_create", "gpd_tcp_tracker_destroy", "gpd_tcp_tracker_run",
                                        "gpd_tcp_tracker_states", "gpd_tcp_tracker_forget", "gpd_tcp_tracker_reset"]
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert sorted(set(re.findall(r"\b(gpd_tcp_tracker_[a-z_]+)\s*\(", code))) == sorted(M.TCPTRACK_EXPORTS)
    for name in M.TCPTRACK_EXPORTS:
        assert hasattr(_lib.lib, name), name
        assert name not in _lib.EXPORTS and name not in tcpasm.TCPASM_EXPORTS
        assert name not in tcpassembly.TCPSEG_EXPORTS
    for cite in ("reassembly/tcpcheck.go:167-246", "reassembly/memory.go:169-206", "TCPOptionCheck", "index_base",
                 "gpd_flow_insert_keys", "AssembleWithContext", "2^32 - 256"):
        assert cite in header, cite
    assert _lib.lib.gpd_abi_version() == 10
    assert "#define GPD_ABI_VERSION 10 " in open(os.path.join(ROOT, "include", "gpd.h")).read()


def test_lazy_reexport_and_build_lists():
    import gopacket_amd
    from gopacket_amd.build import HEADERS, SOURCES
    assert gopacket_amd.tcptrack.NewConnTracker is not None
    assert "tcptrack" in gopacket_amd.__all__
    names = lambda xs: {os.path.basename(x) for x in xs}
    assert "gpd_tcptrack.hip" in names(SOURCES)
    assert {"gpd_tcptrack.h", "gpd_tcptrack_fsm.h", "gpd_radix_sort.h"} <= names(HEADERS)


def test_sort_has_one_copy():
    """The sort kernels live in gpd_radix_sort.h alone; its three users include it."""
    csrc = os.path.join(ROOT, "gopacket_amd", "csrc")
    for f in ("gpd_tcpseg.hip", "gpd_tcptrack.hip", "gpd_ip4reasm.hip"):
        text = open(os.path.join(csrc, f)).read()
        assert '#include "gpd_radix_sort.h"' in text and "void sort_scatter_kernel" not in text, f
        assert not re.search(r"void\s+\w*_scatter_kernel\b", text), f  # no scatter kernel of its own
        assert not re.search(r"\bmatch_digit\b|\bkSortTile\s*=", text), f
    assert open(os.path.join(csrc, "gpd_radix_sort.h")).read().count("void sort_scatter_kernel") == 1


def _csrc_texts():
    csrc = os.path.join(ROOT, "gopacket_amd", "csrc")
    return {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc))
            if f.endswith((".h", ".hip", ".cpp"))}


def test_gather_has_one_copy():
    """The 16-byte gather's chunk loop is one kernel, in gpd_gather.h; the three stream stages
    include it and none defines a __global__ gather of its own (the stream assembly's is folded in
    too: there is no fallback kernel)."""
    texts = _csrc_texts()
    defs = {f: re.findall(r"__global__[^;{]*?\b(\w*gather\w*)\s*\(", t) for f, t in texts.items()}
    assert {f: d for f, d in defs.items() if d} == {"gpd_gather.h": ["gather_kernel"]}
    for f in ("gpd_ip4reasm.hip", "gpd_tcpasm.hip", "gpd_tcpstream.hip"):
        assert '#include "gpd_gather.h"' in texts[f], f
        assert not re.search(r"struct\s+(GRec|GaArgs|GatherRec)\b|kGatherWaves\s*=|__builtin_nontemporal_store", texts[f]), f
    from gopacket_amd.build import HEADERS
    assert "gpd_gather.h" in {os.path.basename(h) for h in HEADERS}


def test_host_helpers_have_one_copy():
    """One error-return macro per message format (GPD_TRY in gpd_internal.h, HIP_TRY in
    gpd_ctx.h), one up16 and one grow."""
    texts = _csrc_texts()
    macros = {f: re.findall(r"#\s*define\s+(\w*_TRY)\s*\(", t) for f, t in texts.items()}
    assert {f: m for f, m in macros.items() if m} == {"gpd_ctx.h": ["HIP_TRY"], "gpd_internal.h": ["GPD_TRY"]}
    assert '"%s: %s", #expr' in texts["gpd_internal.h"] and '"%s failed: %s", #expr' in texts["gpd_ctx.h"]
    for pat in (r"\bsize_t\s+up16\s*\(", r"\bbool\s+grow\s*\("):
        assert {f: len(re.findall(pat, t)) for f, t in texts.items() if re.search(pat, t)} == {"gpd_internal.h": 1}, pat


def test_struct_layouts_and_constants_match_c(tmp_path):
    from gopacket_amd import tcpassembly
    from gopacket_amd import tcptrack as M
    consts = (("GPD_TCP_STATE_CLOSED", M.TCPStateClosed), ("GPD_TCP_STATE_SYN_SENT", M.TCPStateSynSent),
              ("GPD_TCP_STATE_ESTABLISHED", M.TCPStateEstablished), ("GPD_TCP_STATE_CLOSE_WAIT", M.TCPStateCloseWait),
              ("GPD_TCP_STATE_LAST_ACK", M.TCPStateLastAck), ("GPD_TCP_STATE_RESET", M.TCPStateReset),
              ("GPD_TCP_V_ACCEPT", M.V_ACCEPT), ("GPD_TCP_V_DIR", M.V_DIR), ("GPD_TCP_V_STATE_SHIFT", M.V_STATE_SHIFT),
              ("GPD_TCP_V_STATE_MASK", M.V_STATE_MASK), ("GPD_TCP_V_FSM_DIR", M.V_FSM_DIR),
              ("GPD_TCP_UNTRACKED", M.UNTRACKED), ("GPD_TCP_C_STATE_MASK", M.C_STATE_MASK),
              ("GPD_TCP_C_FSM_DIR", M.C_FSM_DIR), ("GPD_FLOW_NONE", M.FLOW_NONE))
    assert (M.V_ACCEPT, M.V_DIR, M.V_STATE_MASK, M.V_FSM_DIR, M.UNTRACKED, M.C_FSM_DIR) == (1, 2, 0x1C, 0x20, 0xFF, 8)
    assert [M.state_name(s) for s in range(7)] == list(TR.STATE_NAMES) + ["?"]
    assert (M.TCPStateClosed, M.TCPStateReset) == (TR.TCPStateClosed, TR.TCPStateReset) and M.UNTRACKED == TR.UNTRACKED
    exprs = ["sizeof(gpd_tcp_track_opts)", "offsetof(gpd_tcp_track_opts, support_missing_establishment)",
             "offsetof(gpd_tcp_track_opts, reserved)"] + [f"(size_t){n}" for n, _ in consts]
    want = [8, 0, 4] + [v for _, v in consts]
    prog = tmp_path / "t.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gpd_tcptrack.h"\nint main(void){' +
                    "".join(f'printf("%zu\\n", {e});' for e in exprs) + "return 0;}\n")
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    got = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert got == want
    assert C_sizeof(M.GpdTcpTrackOpts) == 8 and M.GpdTcpTrackOpts.reserved.offset == 4
    # the exported kernel constants are the sources'
    src = open(os.path.join(ROOT, "gopacket_amd", "csrc", "gpd_tcptrack.hip")).read()
    threads = int(re.search(r"kTrkThreads = (\d+);", src).group(1))
    items = int(re.search(r"kTrkItems = (\d+);", src).group(1))
    assert M.SCAN_TILE == threads * items and M.AGG_ROUND == int(re.search(r"kAggRound = (\d+);", src).group(1))
    sort = open(os.path.join(ROOT, "gopacket_amd", "csrc", "gpd_radix_sort.h")).read()
    assert tcpassembly.SORT_TILE == int(re.search(r"kSortThreads = (\d+);", sort).group(1)) * \
        int(re.search(r"kSortRounds = (\d+);", sort).group(1))


def C_sizeof(t):
    import ctypes
    return ctypes.sizeof(t)


# ---------------------------------------------------------------- the step function and the maps, on the host
@pytest.fixture(scope="module")
def fsm_host(tmp_path_factory):
    exe = tmp_path_factory.mktemp("fsm") / "tcptrack_fsm_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "c", "tcptrack_fsm_host.cpp"),
                    "-o", str(exe)], check=True)
    return str(exe)


def test_step_function_equals_the_model_everywhere(fsm_host):
    """All 2 x 12 x 32 inputs of the kernels' step function, printed by a stand-alone program
    built with AddressSanitizer and UBSan, against CheckState restated in Python."""
    r = subprocess.run([fsm_host, "table"], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    got = [tuple(map(int, line.split())) for line in r.stdout.splitlines()]
    want = [(o,) + row for o in (0, 1) for row in sorted(TR.step_table(bool(o)), key=lambda t: (t[1], t[0], t[2]))]
    assert len(got) == 2 * 12 * 32 and got == want
    reached = {(o, s) for o, _, _, _, s, _, _ in got}
    assert reached == {(o, s) for o in (0, 1) for s in range(6)}  # every state is some step's result


@pytest.mark.parametrize("seed", [1, 2])
def test_composed_prefix_maps_equal_sequential_steps(fsm_host, seed):
    """Random sequences of 1..300 packets: verdicts from composed prefix maps — as a left fold, as
    a balanced tree, and in pieces cut at arbitrary points and seeded from the carried state —
    equal CheckState run packet after packet (checked inside the sanitized program)."""
    r = subprocess.run([fsm_host, "scan", str(seed), "1500"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok 3000", (r.stdout[-2000:], r.stderr[-2000:])


# ---------------------------------------------------------------- the host part, sanitized
def test_host_error_paths_under_host_sanitizers(tmp_path):
    """tests/c/tcptrack_errpath.cpp: a stand-alone program (its own main, the context and the flow
    table stubbed) linked with gpd_tcptrack.hip, host code built with AddressSanitizer and UBSan,
    run on the CPU against every path of the entry points that returns before a device is needed."""
    from gopacket_amd.build import ARCH, CSRC, HIPCC
    exe = tmp_path / "tcptrack_errpath"
    subprocess.run([HIPCC, f"--offload-arch={ARCH}", "-std=c++17", "-O1", "-g", "-I", os.path.join(ROOT, "include"),
                    "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "c", "tcptrack_errpath.cpp"),
                    os.path.join(CSRC, "gpd_tcptrack.hip"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.stdout, r.stderr)


def test_keep_mask_and_names():
    torch = pytest.importorskip("torch")
    from gopacket_amd import tcptrack as M
    v = torch.tensor([1 | 4, 0 | 4, 0xFF, 1 | 2 | 8, 0x14], dtype=torch.uint8)
    r = M.TrackResult(v, None, 4, 2, 2, 1)
    assert M.keep_mask(r).tolist() == [1, 0, 1, 1, 0] and M.keep_mask(r, untracked=False).tolist() == [1, 0, 0, 1, 0]
    assert M.keep_mask(r).dtype == torch.uint8
    assert list(M.verdict_state(v.numpy()[:2])) == [1, 1]
