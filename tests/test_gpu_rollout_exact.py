"""GPU: the batched fp16 rollout step (k_rollout_band) bit for bit against its
exact restatement (oracle.rollout_chain_f16 over orc_rollout_step_f16).

The kernel header pins the arithmetic per cell: p = sum_s fmaf(T, b, p) in
ascending stencil order from 0, v = p * fl(L_z * fl(1 / max)), stored as
fp16(v); stored fp16 subnormals are values, in the next step's input and in
every statistic.  So for every case and EVERY copy:
  * r.belief(c) equals float32(float64(h) / sum float64(h)) of the emulated
    final plane h bit for bit (assert_array_equal; the cells in the fp16
    subnormal range included);
  * rewards and obs_prob are within rel 1e-5 of the float64 values of the
    emulated planes (<B_k, R_u> / S_k and S_{k+1} M_k / S_k), leaf_upper within
    1e-5 of float64 dots of the emulated final plane -- the bound
    test_rollout_leaf_dots uses for an fp32 sum over such planes.
tests/test_oracle.py::test_rollout_exact_cases_are_sensitive asserts on the
emulated planes alone that each case holds what it is here for (mass in the
last column, on both sides of segment boundaries and band seams, >= 10 % of
the positive stored cells fp16-subnormal).

Which case reaches which branch (copies 13, depth 3 unless the name says
otherwise; every geometry runs from the uniform root and from one-hot roots at
cell (0, 0), at cell (H-1, W-1) and, where W > 256, at columns 255 and 256 of a
middle row):
  * full-coded source (uploaded T with an off-support entry, the stay action
    in the batch): 37x50-offsupport, 5x264-offsupport;
  * dense source against the exact reference, at 16-B and 4-B staged shapes:
    every geometry with TUNE_CODED_MODEL = 0, and the automatic fall-back
    (dictionary overflow) in 37x50-overflow, 5x264-overflow;
  * multi-segment grids with 4-B staging (wp % 8 == 4, W > 256): 3x300
    (44-cell second segment), 70x260 (4-cell second segment);
  * a second segment of a few cells: 5x264 (8 cells, 16-B), 70x260 (4 cells);
  * H smaller than the ring: 1x9 (4-B staging), 2x16 (16-B), 3x300;
  * fewer copies than a chunk: 33x64-copies1, -copies2, -copies3 (and
    -copies5: a full chunk and a 1-copy one);
  * depth 1 (the only step reads the shared root image, istride = 0):
    33x64-depth1; depth 2: 33x64-depth2;
  * band geometry: 33x64 (second band of one row), 70x260 (three bands, the
    last of 6 rows, idle waves), 64x256 (exactly one segment, two full
    bands), 35x512 (two full segments, edge dwords in both directions);
  * every action's sparse template instance: 33x64-nine-actions (nine
    partial chunks), 33x64-same-action (one action, 3 full chunks + 1);
  * PP2_BAND_DMA16=0 on 37x50 and 35x512: bit-identical to the default."""
import numpy as np
import pytest

import rollout_exact_cases as RC
from conftest import GAMMA

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pp2():
    import path_planning_2d_amd as P
    assert P.device_count() >= 1, "no GPU visible"
    return P


def describe(got, want, plane, H, W):
    """Where a belief differs from the emulated one: counts, how many of the
    cells are fp16-subnormal in the emulated stored plane, the first cells."""
    bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
    sub = (plane[bad] > 0) & (plane[bad].astype(np.float64) < RC.F16_MIN_NORMAL)
    first = [(int(i // W), int(i % W), float(got[i]), float(want[i])) for i in bad[:4]]
    return (f"{bad.size} of {H * W} cells differ ({int(sub.sum())} of them fp16-subnormal in the "
            f"emulated plane, {int((want[bad] == 0).sum())} zero there); first (y, x, got, want): {first}")


def rel_err(got, want):
    got = np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    return float(np.max(np.abs(got - want) / np.abs(want)))


def run_case(pp2, case, source, compare=True):
    """Run the case on the device with the given model source ("sparse",
    "full", "dense": TUNE_CODED_MODEL = 0, "overflow": automatic dense) and
    compare every run and copy with the emulation.  Returns the device's
    results [(res, beliefs)] per run."""
    inp = RC.inputs(case)
    em = RC.emulate(case) if compare else None
    H, W = case.H, case.W
    problems, out = [], []
    with pp2.GridContext(inp["grid"], inp["goal"], gamma=float(GAMMA)) as ctx:
        ctx.model_generate()
        e_gen, act = ctx.model_dict_info()
        assert act and e_gen > 0
        if case.model != "gen":
            ctx.model_upload(inp["T"], inp["L"], inp["R"], inp["Cc"])
        if source == "dense":
            ctx.set_tuning(ctx.TUNE_CODED_MODEL, 0)
        # which source runs
        entries, active = ctx.model_dict_info()
        if source == "sparse":
            assert case.model == "gen" and active and entries == e_gen
        elif source == "full":  # (at most one more tuple: the off-support cell's)
            assert case.model == "offsupport" and active and e_gen <= entries <= e_gen + 1
        elif source == "dense":
            assert not active
        else:
            assert case.model == "overflow" and (entries, active) == (0, False)
        ctx.fib_set(inp["alphas"])
        with pp2.BatchedRollout(ctx, case.copies, case.depth) as r:
            for name, b0, us, zs in inp["runs"]:
                r.set_root(b0)
                r.run(us, zs)
                res = r.results()
                beliefs = [r.belief(c) for c in range(case.copies)]
                out.append((res, beliefs))
                if not compare:
                    continue
                for c, e in enumerate(em[name]):
                    tag = f"{name} copy {c} (u {us[:, c].tolist()}, z {zs[:, c].tolist()})"
                    if not np.array_equal(beliefs[c].view(np.uint32), e["belief"].view(np.uint32)):
                        problems.append(f"{tag} belief: " + describe(beliefs[c], e["belief"],
                                                                      e["plane"], H, W))
                    for key, got, want in (("rewards", res["rewards"][:, c], e["rewards"]),
                                           ("obs_prob", res["obs_prob"][:, c], e["obs_prob"]),
                                           ("leaf_upper", res["leaf_upper"][c], e["leaf_upper"])):
                        err = rel_err(got, want)
                        if not err <= 1e-5:
                            problems.append(f"{tag} {key}: rel err {err:.3e} (got {got}, want {want})")
    assert not problems, f"{len(problems)} mismatches:\n" + "\n".join(problems[:12])
    return out


@pytest.mark.parametrize("source", ["sparse", "dense"])
@pytest.mark.parametrize("key", list(RC.GEOM_CASES))
def test_rollout_exact_geometry(pp2, key, source):
    run_case(pp2, RC.GEOM_CASES[key], source)


@pytest.mark.parametrize("source", ["sparse", "dense"])
@pytest.mark.parametrize("key", list(RC.EXTRA_CASES))
def test_rollout_exact_batches(pp2, key, source):
    """33 x 64: copies 1, 2, 3, 5; one action for all copies; the nine actions
    in nine partial chunks; depth 1 and 2."""
    case = RC.EXTRA_CASES[key]
    if key == "33x64-nine-actions":
        us = RC.inputs(case)["runs"][0][2]
        assert all(set(row.tolist()) == set(range(9)) for row in us)
    run_case(pp2, case, source)


@pytest.mark.parametrize("key", list(RC.MODEL_CASES))
def test_rollout_exact_uploaded_models(pp2, key):
    """An uploaded T with an off-support entry (full-coded rows; the stay
    action that reads the entry is in the batch) and a perturbed T whose
    dictionary overflows (automatic dense)."""
    case = RC.MODEL_CASES[key]
    if case.model == "offsupport":
        assert (RC.inputs(case)["runs"][0][2] == RC.OFF_ACTION).any()
    run_case(pp2, case, "full" if case.model == "offsupport" else "overflow")


@pytest.mark.parametrize("key", ["37x50", "35x512"])
def test_rollout_exact_dma4_staging(pp2, key, monkeypatch):
    """PP2_BAND_DMA16=0 (4-B LDS-DMA staging forced): exact as well, and bit
    for bit the default staging's results."""
    case = RC.GEOM_CASES[key]
    default = run_case(pp2, case, "sparse", compare=False)
    monkeypatch.setenv("PP2_BAND_DMA16", "0")
    forced = run_case(pp2, case, "sparse")
    for (ra, ba), (rb, bb) in zip(default, forced):
        for k in ra:
            np.testing.assert_array_equal(ra[k], rb[k], err_msg=k)
        for x, y in zip(ba, bb):
            np.testing.assert_array_equal(x, y)
