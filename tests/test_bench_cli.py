"""bench.py's command-line contract (no GPU): what each invocation runs and what a distributed line carries.

VERDICT r04 item 4: `bench.py --gpus N` (N > 1) without --workload must run BASELINE.json configs[3] -- the 1-D block-cyclic
partial-pivot LU over the library's RCCL transport, strong scaling, with `per_rank.ncclCommCount` on the line -- and not the
collective-free GEMM; `--gpus 1` stays the DGEMM of configs[1]."""
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_default_workload_one_gpu_is_the_dgemm():
    assert bench.resolve_run(1, None, None) == ("gemm", "torch", True)


def test_default_workload_several_gpus_is_the_block_cyclic_lu_over_rccl():
    for n in (2, 4, 8):
        wl, tr, defaulted = bench.resolve_run(n, None, None)
        assert (wl, tr, defaulted) == ("lu", "rccl", True)


def test_explicit_choices_are_kept():
    assert bench.resolve_run(8, "gemm", None) == ("gemm", "torch", False)
    assert bench.resolve_run(8, "llt", "rccl") == ("llt", "rccl", False)
    assert bench.resolve_run(2, "lu", None) == ("lu", "rccl", False)  # (round 6: the library's own transport for every distributed factorization)
    assert bench.resolve_run(2, "llt", None) == ("llt", "rccl", False) and bench.resolve_run(2, "lu", "torch") == ("lu", "torch", False)
    assert bench.resolve_run(1, "lu", "rccl") == ("lu", "rccl", False)


def test_per_rank_carries_ncclcommcount_of_every_rank():
    world = 4
    allr = np.array([[101.0, 40.0, 8, world, 32, 2.0e9, 3.5]] * world)
    pr = bench.per_rank_dict(allr, "rccl")
    assert pr["ncclCommCount"] == [world] * world and pr["transport"] == "rccl"
    assert pr["update_and_wait_device_ms"] == [61.0] * world and pr["panels_owned"] == [8] * world


def test_source_wires_the_defaults_into_the_run():
    """the distributed branch is what the resolved names select: lu x world > 1 -> dist_partial_piv_lu with the RCCL transport,
    scaling strong, per_rank on the line"""
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert "args.workload, args.transport, defaulted = resolve_run(args.gpus, args.workload, args.transport)" in src
    assert re.search(r'rccl = F\.RcclTransport\(', src) and "transport=rccl" in src
    assert '"scaling": "strong" if (args.workload in ("lu", "llt") and dist is not None) else "weak"' in src
    assert 'out["per_rank"] = per_rank' in src and "lu_1gpu_same_run" in src


def test_cli_has_full_and_dump_outputs_and_checks_steps():
    import subprocess

    h = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, check=True).stdout
    assert "--full" in h and "--dump-outputs DIR" in h
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True)
    assert r.returncode == 2 and "--steps" in r.stderr


def test_plain_run_leaves_the_extras_to_full():
    """what is not the headline (profiled repetition, roofline, `others`, CPU baselines, distributed extras) runs only with --full"""
    src = open(os.path.join(ROOT, "bench.py")).read()
    for cond in ("if dist is None and args.full:", "if args.full and args.workload == \"gemm\":", "elif args.full and args.workload == \"qr\":",
                 "elif args.full:", "if args.full and dist is None and not args.no_extras:", "if args.full and dist is None and not args.no_cpu:",
                 "and args.full and not args.no_extras:", "if dist is not None and args.workload in (\"lu\", \"llt\") and args.full:"):
        assert cond in src, cond


def test_dump_outputs_whole_sampled_lower_and_budget(tmp_path):
    import torch

    big = torch.randn((2100, 3000), dtype=torch.float64, generator=torch.Generator().manual_seed(1)).t()  # column major, 50 MB
    small = torch.randn((40, 100), dtype=torch.float32, generator=torch.Generator().manual_seed(2)).t()
    spd = torch.randn((300, 300), dtype=torch.float64, generator=torch.Generator().manual_seed(3)).t()
    perm = np.arange(2999, -1, -1, dtype=np.uint64)
    outs = {"big": (big, False), "small": (small, False), "l": (spd, True), "perm": (perm, False), "big_lower": (big[:2100], True)}
    w1 = bench.dump_outputs(str(tmp_path / "a"), outs)
    w2 = bench.dump_outputs(str(tmp_path / "b"), outs)
    assert w1 == w2 and sorted(w1) == ["big.npy", "big_lower.npy", "l.npy", "perm.npy", "small.npy"]
    total = 0
    for f in w1:
        x, y = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert x.dtype in (np.float32, np.float64) and np.array_equal(x, y)  # same positions, same values
        total += x.nbytes
    assert total <= 64 << 20
    assert np.array_equal(np.load(tmp_path / "a" / "small.npy"), small.numpy())
    assert np.load(tmp_path / "a" / "small.npy").dtype == np.float32
    assert np.array_equal(np.load(tmp_path / "a" / "l.npy"), np.tril(spd.numpy()))
    assert np.array_equal(np.load(tmp_path / "a" / "perm.npy"), perm.astype(np.float64))
    # a large output: DUMP_SAMPLE entries at the seeded positions, in column-major order
    s = np.load(tmp_path / "a" / "big.npy")
    assert s.shape == (bench.DUMP_SAMPLE,)
    rng = np.random.default_rng(bench.DUMP_SEED)
    i, j = rng.integers(0, 3000, bench.DUMP_SAMPLE), rng.integers(0, 2100, bench.DUMP_SAMPLE)
    o = np.argsort(j * 3000 + i, kind="stable")
    assert np.array_equal(s, big.numpy()[i[o], j[o]])
    sl = np.load(tmp_path / "a" / "big_lower.npy")
    bl = big[:2100].numpy()
    rng = np.random.default_rng(bench.DUMP_SEED)  # every output draws its positions from the same seed
    i, j = rng.integers(0, 2100, sl.size), rng.integers(0, 2100, sl.size)
    i, j = np.maximum(i, j), np.minimum(i, j)
    o = np.argsort(j * 2100 + i, kind="stable")
    assert np.array_equal(sl, bl[i[o], j[o]])
