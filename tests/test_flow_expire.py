"""Flow expiry (include/gpd_flow_expire.h) on the CPU: the header and the export table, the
constants against a compiled C dump, the model (tests/flow_expire_ref.py) against hand-checked
literals, the slot rules of the kernels (gopacket_amd/csrc/gpd_flow_slots.h) compiled for the host
under the sanitizers, and the entry points' no-device paths."""
import os
import re
import subprocess

import pytest

import flow_expire_ref as ER
from conftest import ROOT


# ---------------------------------------------------------------- the ABI
def test_symbols_exported_and_abi_version_kept():
    from gopacket_amd import _lib
    from gopacket_amd import flowexpire as M
    from gopacket_amd import tcptrack
    header = open(os.path.join(ROOT, "include", "gpd_flow_expire.h")).read()
    assert list(M.FLOWEXPIRE_EXPORTS) == ["gpd_flow_remove", "gpd_flow_expire", "gpd_flow_load"]
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert sorted(set(re.findall(r"\b(gpd_flow_[a-z_]+)\s*\(", code))) == sorted(M.FLOWEXPIRE_EXPORTS)
    for name in M.FLOWEXPIRE_EXPORTS:
        assert hasattr(_lib.lib, name), name
        assert name not in _lib.EXPORTS and name not in tcptrack.TCPTRACK_EXPORTS
    # every entry point cites the reference interface it replaces
    for cite in ("tcpassembly/assembly.go:659-676", "reassembly/memory.go:123-130", "tcpassembly/assembly.go:235-271",
                 "reassembly/tcpassembly.go:1260-1291", "time.Before", "index_base", "gpd_tcp_tracker_forget",
                 "GPD_ERR_INVALID", "ascending"):
        assert cite in header, cite
    assert _lib.lib.gpd_abi_version() == 10
    assert "#define GPD_ABI_VERSION 10 " in open(os.path.join(ROOT, "include", "gpd.h")).read()
    M.flowexpire_lib()
    assert _lib.lib.gpd_flow_expire.argtypes == M.FLOWEXPIRE_EXPORTS["gpd_flow_expire"][1]


def test_lazy_reexport_and_build_lists():
    import gopacket_amd
    from gopacket_amd.build import HEADERS
    assert gopacket_amd.flowexpire.Expire is not None and "flowexpire" in gopacket_amd.__all__
    assert {"gpd_flow_expire.h", "gpd_flow_slots.h"} <= {os.path.basename(x) for x in HEADERS}
    for f in ("Remove", "Expire", "Load", "assembler_hold"):
        assert callable(getattr(gopacket_amd.flowexpire, f))
    assert "tracker.forget(ids" in gopacket_amd.flowexpire.__doc__ and "assembler_hold(a)" in gopacket_amd.flowexpire.__doc__


def test_constants_match_c(tmp_path):
    from gopacket_amd import flowexpire as M
    from gopacket_amd import flows
    consts = (("GPD_FLOW_EXPIRE_PAIRS", M.EXPIRE_PAIRS), ("GPD_FLOW_NONE", flows.FLOW_NONE),
              ("GPD_FLOW_FULL", flows.FLOW_FULL), ("GPD_ERR_INVALID", None))
    prog = tmp_path / "t.c"
    prog.write_text('#include <stdio.h>\n#include "gpd_flow_expire.h"\nint main(void){' +
                    "".join(f'printf("%lld\\n", (long long){n});' for n, _ in consts) + "return 0;}\n")
    exe = tmp_path / "t"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)],
                   check=True)
    got = list(map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()))
    assert got[:3] == [v for _, v in consts[:3]] and M.EXPIRE_PAIRS == 1 and got[3] != 0
    # the slot words of the shared header: the tombstone is non-zero with the fingerprint bits zero
    slots = open(os.path.join(ROOT, "gopacket_amd", "csrc", "gpd_flow_slots.h")).read()
    assert "kSlotFpBits = (1ull << 56) - 1ull;" in slots and "kSlotTomb = 1ull << 56;" in slots
    src = open(os.path.join(ROOT, "gopacket_amd", "csrc", "gpd_flow.hip")).read()
    assert "flow_insert_kernel<false, false>" in src and "flow_insert_kernel<true, true>" in src
    assert '#include "gpd_flow_slots.h"' in src and '#include "gpd_compact.h"' in src


# ---------------------------------------------------------------- the model against hand-checked literals
A, B, C_, D = 0x0A000001, 0x0A000002, 0x0A000003, 0x0A000004


def pool_of(entries):
    p = ER.Pool()
    for key, first, last in entries:
        p.merge({key: {"first": first, "last": last, "packets": last - first + 1, "bytes": 60 * (last - first + 1)}})
    return p


def test_model_key_and_reverse():
    k = ER.key_of(A, B, 1000, 80)
    assert len(k) == 40 and k[0:4] == bytes([10, 0, 0, 1]) and k[16:20] == bytes([10, 0, 0, 2])
    assert k[32:36] == bytes([0x03, 0xE8, 0, 80]) and k[36:40] == bytes([1, 4, 4, 0])
    r = ER.reverse_key(k)
    assert r == ER.key_of(B, A, 80, 1000) and ER.reverse_key(r) == k and r != k
    s = ER.key_of(A, A, 7, 7)
    assert ER.reverse_key(s) == s
    assert ER.key_of(A, B, 1, 2, tp=5) != ER.key_of(A, B, 1, 2)


def test_model_strict_cutoff_and_zero():
    ka, kb, kc = ER.key_of(A, B, 1, 2), ER.key_of(A, C_, 1, 2), ER.key_of(A, D, 1, 2)
    p = pool_of([(ka, 0, 9), (kb, 3, 10), (kc, 5, 11)])
    assert p.expire(0) == set() and len(p) == 3              # last_below = 0 removes nothing
    assert p.expire(9) == set() and len(p) == 3              # 9 < 9 is false: strict, as time.Before
    assert p.expire(10) == {ka} and set(p.flows) == {kb, kc}
    assert p.expire(11) == {kb} and p.expire(11) == set()
    assert p.expire(1 << 62) == {kc} and len(p) == 0
    p.remove([ka, kb])                                       # not in the pool: ignored
    assert len(p) == 0


def test_model_hold_and_recreation():
    ka, kb = ER.key_of(A, B, 1, 2), ER.key_of(A, C_, 1, 2)
    p = pool_of([(ka, 0, 4), (kb, 1, 5)])
    assert p.expire(100, held=[ka]) == {kb} and set(p.flows) == {ka}
    assert p.expire(100, held=[kb]) == {ka}
    # a key that comes back is a new record with fresh counters
    p.merge({ka: {"first": 50, "last": 52, "packets": 2, "bytes": 120}})
    assert p.flows[ka] == {"first": 50, "last": 52, "packets": 2, "bytes": 120}
    p.merge({ka: {"first": 60, "last": 60, "packets": 1, "bytes": 60}})
    assert p.flows[ka] == {"first": 50, "last": 60, "packets": 3, "bytes": 180}


def test_model_pairs():
    c, s = ER.key_of(A, B, 1000, 80), ER.key_of(B, A, 80, 1000)      # a connection's two halves
    lone = ER.key_of(A, C_, 5, 6)                                    # its reverse never appeared
    own = ER.key_of(D, D, 7, 7)                                      # its own reverse
    c2, s2 = ER.key_of(C_, D, 2000, 80), ER.key_of(D, C_, 80, 2000)  # both halves idle
    p = pool_of([(c, 0, 3), (s, 1, 20), (lone, 2, 4), (own, 5, 6), (c2, 7, 8), (s2, 9, 9)])
    q = pool_of([(c, 0, 3), (s, 1, 20), (lone, 2, 4), (own, 5, 6), (c2, 7, 8), (s2, 9, 9)])
    # client half idle, server half recent: neither leaves with pairs, the idle one without
    assert p.expire(10, pairs=True) == {lone, own, c2, s2} and set(p.flows) == {c, s}
    assert q.expire(10) == {c, lone, own, c2, s2} and set(q.flows) == {s}
    # a held half keeps its idle peer
    r = pool_of([(c2, 7, 8), (s2, 9, 9)])
    assert r.expire(10, held=[s2], pairs=True) == set() and r.expire(10, held=[s2]) == {c2}
    # once both are idle they leave together
    assert p.expire(21, pairs=True) == {c, s}


# ---------------------------------------------------------------- the slot rules, on the host
@pytest.fixture(scope="module")
def slots_host(tmp_path_factory):
    exe = tmp_path_factory.mktemp("slots") / "flow_slots_host"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    os.path.join(ROOT, "tests", "c", "flow_slots_host.cpp"), "-o", str(exe)], check=True)
    return str(exe)


@pytest.mark.parametrize("seed", [1, 2])
def test_slot_rules_equal_a_map(slots_host, seed):
    """Random insert, remove and expire-all sequences on tables of 8, 64 and 1024 slots: the shared
    header's find-or-claim, remove and sweep against std::unordered_map (checked inside the
    sanitized program), reaching a full table, claimed tombstones and the no-empty-slot claim."""
    r = subprocess.run([slots_host, str(seed), "4000"], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    m = re.fullmatch(r"ok 12000 full (\d+) tombstones claimed (\d+) after the whole circle (\d+)", r.stdout.strip())
    assert m and all(int(g) > 10 for g in m.groups()), r.stdout


# ---------------------------------------------------------------- the host part, sanitized
def test_host_error_paths_under_host_sanitizers(tmp_path):
    """tests/c/flow_expire_errpath.cpp: a stand-alone program (its own main, the context stubbed,
    the table poisoned) linked with gpd_flow.hip, host code built with AddressSanitizer and UBSan,
    run on the CPU against every path of the entry points that returns before a device is needed."""
    from gopacket_amd.build import ARCH, CSRC, HIPCC
    exe = tmp_path / "flow_expire_errpath"
    subprocess.run([HIPCC, f"--offload-arch={ARCH}", "-std=c++17", "-O1", "-g", "-I", os.path.join(ROOT, "include"),
                    "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "tests", "c", "flow_expire_errpath.cpp"),
                    os.path.join(CSRC, "gpd_flow.hip"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.stdout, r.stderr)
