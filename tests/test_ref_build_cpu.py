"""The recipe that cuts the reference's kernels out by name (oracle/ref_build.py),
on made-up source text: it takes exactly the named definition, is not misled by
braces in comments, and fails loudly instead of building a partial library."""
import os

import pytest

from oracle import ref_build as RB

SRC = """
#include <cuda.h>
void hostOnly(int n) { if (n) { n = 0; } }

__device__
void  helperFn(const float* const __restrict__ a,
    float* const __restrict__ b) {
  // if (a) {   <- an unbalanced brace in a comment
  for (int i = 0; i < 3; ++i) { b[i] = a[i]; }
  /* } */
  return;
}

__global__ void declaredOnly(int n);

__global__
void kernelFn(int n, float* out) {
  //if (n == 3) {
  //  printf("}");
  //}
  if (n > 0) { out[0] = 1.0f; }
}

void launcher() { kernelFn<<<1, 1>>>(1, 0); }
"""


def test_cuts_exactly_the_named_definition():
    k = RB.cut_function(SRC, "kernelFn", "made-up")
    assert k.startswith("__global__\nvoid kernelFn(int n, float* out) {")
    assert k.endswith("if (n > 0) { out[0] = 1.0f; }\n}")
    assert "launcher" not in k and "helperFn" not in k
    h = RB.cut_function(SRC, "helperFn", "made-up")
    assert h.startswith("__device__\nvoid  helperFn(")
    assert h.endswith("return;\n}")
    assert "declaredOnly" not in h


@pytest.mark.parametrize("name", ["missingFn", "hostOnly", "declaredOnly"])
def test_fails_loudly(name):
    """An absent name, a function that is no kernel, a mere declaration."""
    with pytest.raises(SystemExit) as e:
        RB.cut_function(SRC, name, "made-up")
    assert name in str(e.value)


def test_missing_source_file_fails(tmp_path, monkeypatch):
    (tmp_path / "src").mkdir()
    monkeypatch.setenv("PP2_REFERENCE_DIR", str(tmp_path))
    with pytest.raises(SystemExit):
        RB.cut_all(RB.reference_dir())


def test_absent_reference_tree_is_not_an_error(tmp_path, monkeypatch):
    """Nothing is built and nothing under oracle/_ref/ is touched."""
    monkeypatch.setenv("PP2_REFERENCE_DIR", str(tmp_path / "nowhere"))
    before = {f: os.path.getmtime(os.path.join(RB.OUT, f))
              for f in (os.listdir(RB.OUT) if os.path.isdir(RB.OUT) else [])}
    have = all(os.path.exists(RB.lib_path(v)) for v in RB.VARIANTS)
    assert RB.build() is have
    after = {f: os.path.getmtime(os.path.join(RB.OUT, f))
             for f in (os.listdir(RB.OUT) if os.path.isdir(RB.OUT) else [])}
    assert after == before
