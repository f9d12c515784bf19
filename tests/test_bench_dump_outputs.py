"""bench.py --dump-outputs DIR: after the timed steps, what the headline's last step computed (the output ciphertexts of every
AES-128 block and their decryptions) as DIR/<name>.npy in float32 / float64, at most 64 MB, identical from run to run with the
same arguments - so that two builds can be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
sys.path.insert(0, ROOT)
import bench  # noqa: E402


class FakeWires:
    """Row r of the wire table holds the words r * 1000 + j (j < width), large enough to need more than float32."""

    def __init__(self, width):
        self.width = width

    def download(self, rows):
        rows = np.asarray(rows, np.int64)
        return (rows[:, None] * 1000 + np.arange(self.width)[None, :] + 2**31).astype(np.uint32)


class FakeClientKey:
    def decrypt(self, lwe):
        return ((lwe[:, 0].astype(np.int64) - 2**31) // 1000) % 3 == 0


def _layout(blocks, nw=300):
    index = {f"ct[{i}]": 10 + i for i in range(128)}
    return index, nw, blocks


def test_steps_and_dump_arguments():
    a = bench.parse_args(["--steps", "3", "--warmup", "0", "--dump-outputs", "out"])
    assert a.steps == 3 and a.warmup == 0 and a.dump_outputs == "out"
    assert bench.parse_args([]).dump_outputs is None
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse_args(["--warmup", "-1"])


def test_dump_writes_every_block_exactly(tmp_path):
    index, nw, blocks = _layout(4)
    shapes = bench.dump_outputs(str(tmp_path), FakeClientKey(), FakeWires(723), index, nw, blocks)
    assert shapes == {"aes_ct_lwe": [4, 128, 723], "aes_ct_bits": [4, 128], "aes_ct_lwe_blocks": [4]}
    lwe = np.load(tmp_path / "aes_ct_lwe.npy")
    bits = np.load(tmp_path / "aes_ct_bits.npy")
    assert lwe.dtype == np.float64 and bits.dtype == np.float32
    rows = np.array([b * nw + index[f"ct[{i}]"] for b in range(blocks) for i in range(128)])
    want = FakeWires(723).download(rows).reshape(blocks, 128, 723)
    assert np.array_equal(lwe.astype(np.uint32), want) and np.array_equal(lwe, want.astype(np.float64))
    assert np.array_equal(bits, (rows % 3 == 0).reshape(blocks, 128).astype(np.float32))
    assert np.array_equal(np.load(tmp_path / "aes_ct_lwe_blocks.npy"), np.arange(blocks, dtype=np.float64))


def test_dump_of_a_large_table_is_a_fixed_sample_under_the_limit(tmp_path):
    index, nw, blocks = _layout(40)
    limit = 10 * 128 * 723 * 8 + 40 * 128 * 4 + 40 * 8   # room for ten blocks' ciphertexts
    bench.dump_outputs(str(tmp_path / "a"), FakeClientKey(), FakeWires(723), index, nw, blocks, limit=limit)
    bench.dump_outputs(str(tmp_path / "b"), FakeClientKey(), FakeWires(723), index, nw, blocks, limit=limit)
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= limit + 3 * 256   # + the .npy headers
    kept = np.load(tmp_path / "a" / "aes_ct_lwe_blocks.npy").astype(np.int64)
    assert len(kept) == 10 and np.all(np.diff(kept) > 0) and kept[-1] < blocks
    for name in ("aes_ct_lwe", "aes_ct_bits", "aes_ct_lwe_blocks"):
        assert np.array_equal(np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy"))
    lwe = np.load(tmp_path / "a" / "aes_ct_lwe.npy")
    assert np.array_equal(lwe[3, 5].astype(np.uint32), FakeWires(723).download([kept[3] * nw + index["ct[5]"]])[0])
    assert np.load(tmp_path / "a" / "aes_ct_bits.npy").shape == (40, 128)


def test_default_job_fits_the_limit():
    """The default 32-block job at the boolean set (n = 722) is dumped whole: no sampling."""
    assert 32 * 128 * 723 * 8 + 32 * 128 * 4 + 32 * 8 <= bench.DUMP_LIMIT_BYTES


@pytest.mark.gpu
def test_two_runs_dump_the_same_outputs_and_they_decrypt_to_aes(tmp_path):
    from helm_amd.netlists import aes128_reference_encrypt
    args = ["--gpus", "1", "--steps", "2", "--warmup", "0", "--blocks", "2", "--no-cpu-baseline", "--no-other-modes", "--no-configs"]
    for run in ("a", "b"):
        p = subprocess.run([sys.executable, BENCH] + args + ["--dump-outputs", str(tmp_path / run)], stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-3000:]
        line = json.loads(p.stdout.strip().splitlines()[-1])
        assert "error" not in line and line["steps"] == 2 and line["ms_per_step"] > 0
        assert line["dumped_outputs"]["arrays"]["aes_ct_lwe"] == [2, 128, 723]
    for name in ("aes_ct_lwe", "aes_ct_bits", "aes_ct_lwe_blocks"):
        assert np.array_equal(np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")), name
    bits = np.load(tmp_path / "a" / "aes_ct_bits.npy").astype(np.int64)
    # block 0 is FIPS-197 C.1 (bench.py pins it)
    want = aes128_reference_encrypt(bytes(range(16)), bytes.fromhex("00112233445566778899aabbccddeeff"))
    assert sum(int(bits[0, i]) << i for i in range(128)).to_bytes(16, "big") == want
