"""The BPF filter without a GPU: the validator and gpd_bpf_run_host — the interpreter the kernel
runs (gopacket_amd/csrc/gpd_bpf_vm.h), compiled for the host — against the checker
(tests/bpf_ref.py), exact equality everywhere; the Python surface; the kernel's register
metadata; and the same host code from a plain C program under the address and undefined-behaviour
sanitizers."""
import os
import re
import subprocess

import pytest

import bpf_cases as BC
import bpf_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GPD_ERR_INVALID = -1


def _bpf():
    from gopacket_amd import bpf
    return bpf


def run_host(prog, data, wirelen=None):
    B = _bpf()
    _, arr = B._c_program(prog)
    data = bytes(data)
    return B.bpf_lib().gpd_bpf_run_host(arr, len(prog), data, len(data), len(data) if wirelen is None else wirelen)


def validate_rc(prog):
    B = _bpf()
    _, arr = B._c_program(prog)
    rc = B.bpf_lib().gpd_bpf_validate(arr, len(prog))
    from gopacket_amd import _lib
    return rc, _lib.lib.gpd_last_error_string().decode()


# ---- the reference's vector -----------------------------------------------------------------------
def test_reference_packet_vector():
    B = _bpf()
    assert len(BC.PACKET) == 38
    for flt in BC.VEC["filters"]:
        prog = [tuple(q) for q in flt["program"]]
        f = B.NewBPFInstructionFilter([B.BPFInstruction(*q) for q in prog], None)
        for case in flt["cases"]:
            data = BC.PACKET[:case["caplen"]]
            assert R.run(prog, data, len(data)) == case["ret"], flt["name"]
            assert run_host(prog, data) == case["ret"], flt["name"]
            assert f.run(data) == case["ret"]
            # Matches as the benchmarks call it: CaptureLength = Length = len(packet)
            from gopacket_amd.pcapwrite import CaptureInfo
            assert f.Matches(CaptureInfo(0, len(data), len(data)), data) is case["matches"], flt["name"]
    assert BC.VEC["filters"][0]["cases"][0]["ret"] == 262144
    assert f.String() == "BPF Instruction Filter"


# ---- gpd_bpf_run_host == checker -------------------------------------------------------------------
def test_edge_programs_equal_checker():
    packets = BC.edge_packets()
    progs = BC.edge_programs()
    assert len(progs) > 250
    seen_nonzero = 0
    for name, prog in progs:
        for data, wirelen in packets:
            want = R.run(prog, data, wirelen)
            assert run_host(prog, data, wirelen) == want, (name, len(data), wirelen)
            seen_nonzero += want != 0
    assert seen_nonzero > 300  # (the cases are not all failures)


def test_edge_expectations_by_hand():
    """A few of the edges, with the value written out: the checker is checked too."""
    body, _ = BC.edge_packets()[0]
    L = BC.L
    by_name = dict(BC.edge_programs())
    both = lambda name, data, wl=None: (R.run(by_name[name], data, wl), run_host(by_name[name], data, wl))
    assert both(f"ld_w_abs_{L - 4:#x}", body) == (int.from_bytes(body[-4:], "big"),) * 2
    assert both(f"ld_w_abs_{L - 3:#x}", body) == (0, 0)
    assert both(f"ld_h_abs_{L - 2:#x}", body) == (int.from_bytes(body[-2:], "big"),) * 2
    assert both(f"ld_h_abs_{L - 1:#x}", body) == (0, 0)
    assert both(f"ld_b_abs_{L - 1:#x}", body) == (body[-1],) * 2
    assert both(f"ld_b_abs_{L:#x}", body) == (0, 0)
    assert both("ld_b_ind_x0xffffffff_k0x1", body) == (0, 0)  # no wrapped sum
    assert both("ld_w_ind_x0xffffffff_k0x1", body) == (0, 0)
    assert both(f"ld_b_ind_x{L - 1:#x}_k0x0", body) == (body[-1],) * 2
    assert both(f"ld_b_ind_x{L - 1:#x}_k0x1", body) == (0, 0)
    assert both(f"ldx_msh_{L - 1:#x}", body) == ((body[-1] & 0xF) << 2,) * 2
    assert both(f"ldx_msh_{L:#x}", body) == (0, 0)
    assert both("div_x_zero", body) == (0, 0) and both("mod_x_zero", body) == (0, 0)
    assert both("lsh_x_0x1f", body) == (0x80000001,) * 2    # (0x80000001 << 31) + 1
    assert both("lsh_x_0x20", body) == (1, 1) and both("lsh_x_0xffffffff", body) == (1, 1)
    assert both("rsh_x_0x1f", body) == (2, 2) and both("rsh_x_0x20", body) == (1, 1)
    assert both("neg_0", body) == (1, 1) and both("neg_5", body) == (0xFFFFFFFB,) * 2
    assert both("mul_k_wrap", body) == ((0x10001 * 0xFFFF0001) & 0xFFFFFFFF,) * 2
    assert both("ja_to_last", body) == (9, 9)
    assert both("mem_read_before_write", body) == (1, 1)
    assert both("ld_len", body[:5], 1000) == (1000, 1000)
    assert both("ld_len", b"", 77) == (77, 77)             # caplen 0: no packet load, LEN works
    assert both(f"ld_b_abs_{0:#x}", b"", 77) == (0, 0)
    assert both("jgt_k_a0x80000001", body) == (1, 1) and both("jgt_k_a0x7fffffff", body) == (2, 2)
    assert both("jump_255", bytes([0x80])) == (10 + 255,) * 2 and both("jump_255", bytes([0x7F])) == (10, 10)


def test_random_programs_equal_checker():
    for seed in range(200):
        prog = BC.random_program(seed)
        B = _bpf()
        _, arr = B._c_program(prog)
        fn = B.bpf_lib().gpd_bpf_run_host
        for data, wirelen in BC.random_packets(10_000 + seed):
            assert fn(arr, len(prog), data, len(data), wirelen) == R.run(prog, data, wirelen), (seed, data.hex())


def test_random_programs_reach_every_form():
    """The generator's 200 programs, with the edge programs, hold every instruction form."""
    codes = {q[0] for seed in range(200) for q in BC.random_program(seed)}
    codes |= {q[0] for _, prog in BC.edge_programs() for q in prog}
    assert codes == set(R.ALL_CODES)


# ---- the validator ---------------------------------------------------------------------------------
def test_validator_refuses_each_broken_rule():
    for name, prog, idx in BC.invalid_programs():
        rc, text = validate_rc(prog)
        assert rc == GPD_ERR_INVALID, name
        assert f"instruction {idx} " in text, (name, text)
        assert run_host(prog, b"\x01") == 0, name
        with pytest.raises(_bpf().BPFError):
            _bpf().validate(prog)
    for name, prog in BC.edge_programs():
        assert validate_rc(prog)[0] == 0, name


def test_validator_length_rule():
    ok = BC.ret_k(1)
    rc, text = validate_rc([])
    assert rc == GPD_ERR_INVALID and "empty" in text
    rc, text = validate_rc([ok] * 4097)
    assert rc == GPD_ERR_INVALID and "4096" in text
    assert validate_rc([ok] * 4096)[0] == 0
    prog = BC.max_length_program()
    assert len(prog) == 4096 and validate_rc(prog)[0] == 0
    assert R.run(prog, b"") == 4095 and run_host(prog, b"") == 4095
    B = _bpf()
    assert B.bpf_lib().gpd_bpf_validate(None, 1) == GPD_ERR_INVALID


# ---- the Python surface ----------------------------------------------------------------------------
DD = """{ 0x28, 0, 0, 0x0000000c },
{ 0x15, 0, 10, 0x00000800 },
{ 0x30, 0, 0, 0x00000017 },
{ 0x15, 0, 8, 0x00000006 },
{ 0x28, 0, 0, 0x00000014 },
{ 0x45, 6, 0, 0x00001fff },
{ 0xb1, 0, 0, 0x0000000e },
{ 0x48, 0, 0, 0x0000000e },
{ 0x15, 2, 0, 0x00000050 },
{ 0x48, 0, 0, 0x00000010 },
{ 0x15, 0, 1, 0x00000050 },
{ 0x6, 0, 0, 0x00040000 },
{ 0x6, 0, 0, 0x00000000 },
"""


def test_parse_dd_roundtrip_and_error():
    B = _bpf()
    ins = B.parse_dd(DD)
    assert [(i.Code, i.Jt, i.Jf, i.K) for i in ins] == BC.PORT80
    assert B.format_dd(ins) == DD and B.parse_dd(B.format_dd(ins)) == ins
    assert B.parse_dd("\n  { 6, 0, 0, 7 }\n\n") == [B.BPFInstruction(6, 0, 0, 7)]
    for bad in ("{ 0x28, 0, 0 },", "(000) ldh [12]", "{ 0x28, 0, 0, 0x0000000c }, extra", "{ 0x28, 256, 0, 0 },",
                "{ 0x28, 0, 0, 0x100000000 },"):
        with pytest.raises(ValueError) as e:
            B.parse_dd(DD + bad + "\n")
        assert "line 14" in str(e.value)


def test_expression_compiler_is_not_here():
    B = _bpf()
    for fn in (B.NewBPF, B.CompileBPFFilter):
        with pytest.raises(NotImplementedError) as e:
            fn("ip and tcp and port 80")
        assert "tcpdump -dd" in str(e.value) and "port 80" in str(e.value)


def test_host_only_filter_has_no_device_path():
    B = _bpf()
    f = B.NewBPFInstructionFilter(BC.PORT80, None)
    assert f.Matches(None, BC.PACKET) is True
    with pytest.raises(RuntimeError):
        f.match_device(None)
    with pytest.raises(B.BPFError):
        B.NewBPFInstructionFilter([(0xFFFF, 0, 0, 0)], None)
    with pytest.raises(B.BPFError):
        B.NewBPFInstructionFilter([(6, 0, 0, 1 << 32)], None)  # K does not fit 32 bits


def test_new_symbols_exported_and_abi_version_kept():
    from gopacket_amd import _lib
    B = _bpf()
    header = open(os.path.join(ROOT, "include", "gpd_bpf.h")).read()
    B.bpf_lib()
    for name in B.BPF_EXPORTS:
        assert hasattr(_lib.lib, name), name
        assert name + "(" in header, name
        assert name not in _lib.EXPORTS
    assert _lib.lib.gpd_abi_version() == 10
    import gopacket_amd
    assert gopacket_amd.bpf.NewBPFInstructionFilter is not None
    from gopacket_amd.build import HEADERS, KERNEL_SOURCES, SOURCES
    names = lambda paths: {os.path.basename(p) for p in paths}
    assert {"gpd_bpf.hip", "gpd_bpf_host.cpp"} <= names(SOURCES)
    assert {"gpd_bpf.h", "gpd_bpf_vm.h"} <= names(HEADERS)
    assert not any("bpf" in n for n in names(KERNEL_SOURCES))


# ---- the kernel's registers ------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_filter_kernels_do_not_spill(tmp_path):
    """No instance spills a VGPR or has a private segment.  The instance for programs without M
    has no LDS either: M costs its own instance 16 x 256 words of LDS and the other nothing."""
    out = tmp_path / "bpf.s"
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I",
                    os.path.join(ROOT, "include"), "-S", "--cuda-device-only",
                    os.path.join(ROOT, "gopacket_amd", "csrc", "gpd_bpf.hip"), "-o", str(out)],
                   check=True, capture_output=True, timeout=600)
    seen = set()
    for b in out.read_text().split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", b).group(1)
        m = re.search(r"bpf_kernelILb([01])E", name)
        if not m:
            continue
        field = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", b).group(1))
        mem = m.group(1) == "1"
        seen.add(mem)
        assert field("vgpr_spill_count") == 0, name
        assert field("sgpr_spill_count") == 0, name
        assert field("private_segment_fixed_size") == 0, name
        assert field("group_segment_fixed_size") == (4 * 256 * 16 if mem else 0), name
    assert seen == {False, True}, seen


# ---- the host code under the sanitizers ------------------------------------------------------------
def _cases_file(path):
    """Every edge program over the edge packets, 40 random programs, the max-length program and
    the invalid programs, with the checker's expectations."""
    with open(path, "w") as fh:
        def emit(prog, packets, bad=None):
            fh.write(f"prog {len(prog)} {0 if bad is not None else 1} {bad or 0} {len(packets) if bad is None else 0}\n")
            fh.write("".join(f"{c} {jt} {jf} {k}\n" for c, jt, jf, k in prog))
            if bad is None:
                for data, wl in packets:
                    fh.write(f"{wl} {R.run(prog, data, wl)} {len(data)} {data.hex() or '-'}\n")
        n = 0
        for _, prog in BC.edge_programs():
            emit(prog, BC.edge_packets())
            n += 1
        for seed in range(40):
            emit(BC.random_program(seed), BC.random_packets(10_000 + seed, 16))
            n += 1
        emit(BC.max_length_program(), [(b"", 0), (b"\x01", 9)])
        n += 1
        for _, prog, idx in BC.invalid_programs():
            emit(prog, [], bad=idx)
            n += 1
        emit([], [], bad=0)
        emit([BC.ret_k(1)] * 4097, [], bad=0)
        return n + 2


def test_host_code_clean_under_sanitizers(tmp_path):
    """tests/c/bpf_host.c: built from gopacket_amd/csrc/gpd_bpf_host.cpp alone with
    -fsanitize=address,undefined, run as a program of its own."""
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    probe = tmp_path / "probe.c"
    probe.write_text("int main(void) { return 0; }\n")
    if subprocess.run(["gcc", *flags, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode:
        flags = []  # no sanitizer runtimes on this machine: the plain build still compares every value
    print("bpf_host flags:", flags or "plain")
    exe, obj = tmp_path / "bpf_host", tmp_path / "bpf_host.o"
    inc = ["-I", os.path.join(ROOT, "include")]
    subprocess.run(["gcc", "-O1", "-g", "-std=c11", "-Wall", *flags, *inc, "-c", os.path.join(HERE, "c", "bpf_host.c"),
                    "-o", str(obj)], check=True, capture_output=True, timeout=120)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", *flags, *inc, "-DGPD_BPF_STANDALONE",
                    os.path.join(ROOT, "gopacket_amd", "csrc", "gpd_bpf_host.cpp"), str(obj), "-o", str(exe)],
                   check=True, capture_output=True, timeout=120)
    cases = tmp_path / "cases.txt"
    nprog = _cases_file(cases)
    r = subprocess.run([str(exe), str(cases)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    words = r.stdout.split()
    assert words[:2] == ["bpf_host", "ok"] and int(words[2]) == nprog and int(words[3]) > 1500, r.stdout
    assert r.stderr == ""
