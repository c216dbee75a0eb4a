"""bench.py's plain one-GPU run: only the timed steps and the result line, and `--dump-outputs`
writes what the last timed step computed — checked word for word against the oracle's decode of
the same seeded batch."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FULL_ONLY = ("record36", "record36_aos", "record_soa", "record_aos", "fallback", "pcie_inclusive",
             "pcie_diag_rank0", "cpu_baseline", "tcp64", "imix", "vxlan", "pcap64")


def test_dump_sample_is_fixed_and_bounded():
    import bench
    n = 1 << 24
    rows = bench.dump_rows(n)
    assert len(rows) == bench.DUMP_SAMPLE and np.array_equal(rows, bench.dump_rows(n))
    assert np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < n
    assert np.array_equal(bench.dump_rows(1000), np.arange(1000))
    # index, status, csum: one float64 per packet; layers, net_hash, tp_hash: two
    assert bench.DUMP_SAMPLE * 9 * 8 <= 64 * 10 ** 6


def _plain(tmp_path, config, n):
    """One plain run (3 steps, 1 warmup) with --dump-outputs: (the line, {name: array})."""
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3",
                        "--warmup", "1", "--settle-ms", "20", "--config", config, "--packets", str(n),
                        "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=120, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    d = json.loads(lines[0])
    assert d["unit"] == "Mpackets/s" and d["higher_is_better"] is True and d["dtype"] == "u8"
    assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1 and d["ms_per_step"] > 0
    assert abs(d["value"] - n / (d["ms_per_step"] * 1e-3) / 1e6) <= 0.02 * d["value"]
    assert not [k for k in FULL_ONLY if k in d] and "attainable" not in d["roofline"]
    assert d["outputs"]["packets"] == n
    return d, {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}


def _assert_dump_is(got, ref, n):
    assert sorted(got) == ["csum", "index", "layers", "net_hash", "status", "tp_hash"]
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["index"], np.arange(n))
    for f in ("status", "csum"):
        assert np.array_equal(got[f], getattr(ref, f).astype(np.float64)), f
    for f in ("layers", "net_hash", "tp_hash"):
        w = getattr(ref, f)
        assert np.array_equal(got[f][:, 0], (w & np.uint64(0xFFFFFFFF)).astype(np.float64)), f
        assert np.array_equal(got[f][:, 1], (w >> np.uint64(32)).astype(np.float64)), f


@pytest.mark.gpu
@pytest.mark.parametrize("config,n", [("udp64", (1 << 16) + 3), ("imix", 20001)])
def test_plain_line_and_dumped_outputs(tmp_path, config, n):
    """gpd_records (udp64) and the SoA arrays (imix); n is no multiple of the 64-packet tile."""
    import bench
    import oracle_ref as O
    d, got = _plain(tmp_path, config, n)
    assert d["config"]["packets_per_gpu"] == n and d["config"]["decode_errors_in_batch"] == 0
    _assert_dump_is(got, O.decode(bench.make_batch(config, n, 0), ext=False), n)  # bench.py's decoder set


@pytest.mark.gpu
def test_plain_replay_line_and_dumped_outputs(tmp_path):
    """Config 5 without --full: the resident leg alone (no streamed leg, none of its figures); its
    records are config 2's packets, so the dumped words equal the oracle's for those."""
    import bench
    import oracle_ref as O
    from gopacket_amd import synth
    n = 100003
    d, got = _plain(tmp_path, "replay", n)
    assert d["scaling"] == "strong" and d["config"]["packets_total"] == n and d["config"]["decode_errors"] == 0
    assert set(d["per_rank"][0]) == {"rank", "packets", "kernel_ms_per_step", "frac", "read_frac",
                                     "decode_errors", "registered"}
    _assert_dump_is(got, O.decode(synth.make_udp64(n, bench.REPLAY_SEED), ext=False), n)
