"""CPU: the ABI and the Python mirror of the lookahead that follows a batch's
placement (pp2_episodes_run_lookahead_placed; ``placed=True``) -- no GPU.

* include/pp2.h declares the new entry, keeps the old entry's contract text
  and PP2_ABI_VERSION 4 (the addition is additive);
* ``_lib`` binds it with five arguments and the built library exports it;
* ``EpisodeBatch.run_lookahead`` and ``EpisodeBatch.run`` accept ``placed``,
  route it to the new call, and reject a non-bool before they touch the
  library.
"""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest


def test_header_declares_the_placed_lookahead():
    from path_planning_2d_amd import _lib
    text = open(_lib.HEADER_PATH).read()
    assert re.search(r"^#define PP2_ABI_VERSION 4\b", text, re.M) and _lib.PP2_ABI_VERSION == 4
    flat = re.sub(r"\s+", " ", text)
    assert ("int pp2_episodes_run_lookahead_placed(pp2_episodes* ep, int alpha_set, uint64_t seed, "
            "const float* b0, const int32_t* start_cells);") in flat
    # the old entry is still declared, with its contract
    assert ("int pp2_episodes_run_lookahead(pp2_episodes* ep, int alpha_set, uint64_t seed, "
            "const float* b0, const int32_t* start_cells);") in flat
    flat = flat.replace(" * ", " ")
    assert ("PP2_EINVAL before any launch also when the workgroup's LDS with the lookahead "
            "scratch does not fit -- also on a PP2_EPISODES_AUTO batch -- and on every "
            "PP2_EPISODES_GLOBAL batch: the lookahead runs from LDS planes only.") in flat
    assert "Lookahead runs (pp2_episodes_run_lookahead)" in text


def test_lib_binds_and_the_library_exports_it():
    from path_planning_2d_amd import _lib
    sig = _lib.SIGNATURES["pp2_episodes_run_lookahead_placed"]
    assert len(sig) == 5
    assert sig == _lib.SIGNATURES["pp2_episodes_run_lookahead"]
    path = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "libpp2_hip.so")
    assert os.path.exists(path), "the library is not built"
    lib = C.CDLL(path)
    assert hasattr(lib, "pp2_episodes_run_lookahead_placed")
    assert hasattr(lib, "pp2_episodes_run_lookahead")


def bare_batch():
    """An EpisodeBatch without a context or a library handle: any call of the
    library through it fails on ``_h`` (None)."""
    from path_planning_2d_amd import EpisodeBatch
    ep = EpisodeBatch.__new__(EpisodeBatch)
    ep._h, ep.cells, ep.episodes = None, 12, 3
    return ep


def test_signatures_accept_placed():
    from path_planning_2d_amd import EpisodeBatch
    for fn in (EpisodeBatch.run_lookahead, EpisodeBatch.run):
        p = inspect.signature(fn).parameters
        assert list(p)[-2:] == ["seed", "placed"], fn
        assert p["placed"].default is False and p["seed"].default == 0


def test_placed_is_validated_and_routed_before_the_library(monkeypatch):
    from path_planning_2d_amd import episodes as E
    ep = bare_batch()
    b0 = np.full(12, 1 / 12, np.float32)
    starts = [0, 5, 11]
    called = []
    monkeypatch.setattr(E, "call", lambda name, *a: called.append(name))
    for bad in (1, 0, None, "yes", "global", np.bool_(True), 1.0, [True]):
        with pytest.raises(ValueError, match="placed"):
            ep.run_lookahead("fib", b0, starts, 0, bad)
        for policy in ("fib-lookahead", "pbvi-lookahead", "qmdp", "mode", "fib", "pbvi"):
            with pytest.raises(ValueError, match="placed"):
                ep.run(policy, b0, starts, 0, placed=bad)
    assert not called  # nothing reached the library
    # the two lookahead names and run_lookahead go to the new call ...
    assert ep.run_lookahead("fib", b0, starts, 7, placed=True) is ep
    assert ep.run("pbvi-lookahead", b0, starts, 7, placed=True) is ep
    assert ep.run("fib-lookahead", b0, starts, placed=True) is ep and ep.lookahead
    assert called == ["pp2_episodes_run_lookahead_placed"] * 3
    # ... the default stays the old one, and the other policies' calls do not change
    del called[:]
    ep.run_lookahead("pbvi", b0, starts)
    ep.run("fib-lookahead", b0, starts, 3, False)
    for placed in (False, True):
        ep.run("qmdp", b0, starts, 1, placed)
        ep.run("mode", b0, starts, placed=placed)
        ep.run("fib", b0, starts, placed=placed)
        ep.run("pbvi", b0, starts, placed=placed)
    assert called == ["pp2_episodes_run_lookahead"] * 2 + [
        "pp2_episodes_run", "pp2_episodes_run", "pp2_episodes_run_alpha",
        "pp2_episodes_run_alpha"] * 2
    # the other argument checks still come before the library
    del called[:]
    with pytest.raises(ValueError):
        ep.run_lookahead("fib", b0[:11], starts, 0, True)
    with pytest.raises(ValueError):
        ep.run_lookahead("greedy", b0, starts, 0, True)
    assert not called
