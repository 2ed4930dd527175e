"""bench.py command line: result line, --full, --dump-outputs (CPU engine,
tiny row count, in-process)."""

import json
import os
import sys

import numpy as np

import bench


def run_bench(monkeypatch, capsys, tmp_path, *extra):
    monkeypatch.setattr(sys, "argv", [
        "bench.py", "--gpus", "1", "--engine", "cpu", "--rows", "300",
        "--dir", str(tmp_path), *extra])
    bench.main()
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 1
    return json.loads(lines[0])


def load_dir(d):
    return {f: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_result_line_and_full(monkeypatch, capsys, tmp_path):
    for extra in ((), ("--full",)):
        r = run_bench(monkeypatch, capsys, tmp_path, "--steps", "3",
                      "--warmup", "1", *extra)
        assert r["steps"] == 3 and r["warmup"] == 1
        assert r["unit"] == "rows/s" and r["higher_is_better"] is True
        assert r["ms_per_step"] > 0
        # value and ms_per_step describe the same timed window
        assert np.isclose(r["value"], 300 / (r["ms_per_step"] / 1000))


def test_dump_outputs_reproducible_and_exact(monkeypatch, capsys, tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    run_bench(monkeypatch, capsys, tmp_path, "--steps", "2", "--warmup", "0",
              "--dump-outputs", a)
    run_bench(monkeypatch, capsys, tmp_path, "--steps", "1", "--warmup", "2",
              "--full", "--dump-outputs", b)
    da, db = load_dir(a), load_dir(b)
    assert list(da) == list(db) and "file_image.npy" in da
    for name in da:
        assert da[name].dtype in (np.float32, np.float64)
        assert np.array_equal(da[name], db[name]), name
    # nothing sampled at this size: the dump is the decoded input, exactly
    src = bench.make_batch(300, seed=1234)
    ids = (da["id.values.hi32.npy"].astype(np.int64) << 32) \
        | da["id.values.lo32.npy"].astype(np.int64)
    assert np.array_equal(ids, src.columns[0].values)
    assert np.array_equal(da["ints.values.npy"], src.columns[1].values)
    assert np.array_equal(da["floats.values.npy"], src.columns[2].values)
    assert np.array_equal(da["tokens.values.npy"], src.columns[3].values)
    assert np.array_equal(da["tokens.elem_off.npy"], src.columns[3].elem_off)


def test_dump_outputs_sampling_is_seeded_and_bounded(monkeypatch, tmp_path):
    monkeypatch.setattr(bench, "_DUMP_BUDGET", 64 * 1024)
    src = bench.make_batch(2000, seed=5)
    f = tmp_path / "img.bin"
    f.write_bytes(bytes(range(256)) * 400)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(a, src, str(f))
    bench.dump_outputs(b, src, str(f))
    da, db = load_dir(a), load_dir(b)
    assert sum(x.nbytes for x in da.values()) <= 2 * 64 * 1024
    assert da["floats.values.npy"].size < src.columns[2].values.size
    for name in da:
        assert np.array_equal(da[name], db[name]), name
