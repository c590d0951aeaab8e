"""Builds the reference's own per-cell kernels for the host, into ``oracle/_ref/``.

TEST INFRASTRUCTURE ONLY (see ``pp2_oracle.h``).  The reference's host code
needs nvcc, ROS and Boost, but the kernels named below are plain C++ behind
``ref_shim.h``.  This recipe names files and functions and nothing more: at
build time it cuts each named definition out of the reference tree, writes
the cut text to ``oracle/_ref/`` (ignored by git) and compiles
``ref_driver.cpp`` around it into two libraries,

    libpp2_ref_fma.so    -O2 -ffp-contract=fast -mfma -fno-fast-math
    libpp2_ref_nofma.so  the same with -ffp-contract=off

for a fixed x86-64-v3 baseline (no -march=native: the libraries are built on
one machine and loaded on another).  ``oracle/ref.py`` loads them.

The reference tree is looked for in ``$PP2_REFERENCE_DIR``, else in
``reference/path_planning_2d`` beside the repository.  Where it is absent
nothing is built and an existing ``oracle/_ref/`` is left as it is.
"""
from __future__ import annotations

import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "_ref")
DEFAULT_REF = os.path.join(os.path.dirname(os.path.dirname(HERE)), "reference",
                           "path_planning_2d")

# namespace -> [(source file, [function names])]; the MDP and POMDP sources
# reuse names, so each set becomes an include file of its own
KERNELS = {
    "ref_mdp": [
        ("src/mdp/path_planning_2d_cuda.cu",
         ["cudaTransitionProbability", "cudaStageCost", "cudaGenerateModelData",
          "cudaOneStepValueIteration"]),
    ],
    "ref_pomdp": [
        ("src/pomdp/model_generation_cuda.cu",
         ["cudaTransitionProbability", "cudaMeasurementLikelihood", "cudaStageReward",
          "cudaGenerateModelData"]),
        ("src/pomdp/point_based_value_iteration_cuda.cu",
         ["cudaBayesBeliefUpdate", "cudaComputeGammaOA"]),
        ("src/pomdp/fast_informed_bound_cuda.cu", ["cudaFIBValueIteration"]),
    ],
}

BASE_FLAGS = ["-O2", "-march=x86-64-v3", "-mfma", "-fno-fast-math", "-std=c++14", "-fPIC",
              "-shared", "-w"]
VARIANTS = {"fma": "-ffp-contract=fast", "nofma": "-ffp-contract=off"}


def lib_path(variant: str) -> str:
    return os.path.join(OUT, f"libpp2_ref_{variant}.so")


def reference_dir() -> str:
    return os.environ.get("PP2_REFERENCE_DIR") or DEFAULT_REF


def _blank_comments(text: str) -> str:
    """`text` with comments and string / character literals overwritten by
    spaces (same length), so that braces can be counted on what is left."""
    pat = re.compile(r"//[^\n]*|/\*.*?\*/|\"(?:\\.|[^\"\\\n])*\"|'(?:\\.|[^'\\\n])*'", re.S)
    return pat.sub(lambda m: re.sub(r"[^\n]", " ", m.group(0)), text)


def cut_function(text: str, name: str, where: str) -> str:
    """The definition of the __global__ / __device__ function `name`: from
    its qualifier to the brace that closes its body."""
    code = _blank_comments(text)
    found = [m for m in re.finditer(
        r"__(?:global|device)__\s+void\s+" + re.escape(name) + r"\s*\(", code)]
    if len(found) != 1:
        raise SystemExit(f"ref_build: {len(found)} definitions of {name} in {where} "
                         f"(expected exactly one)")
    start = found[0].start()
    depth, i = 0, found[0].end() - 1
    while True:  # the parameter list
        c = code[i]
        depth += (c == "(") - (c == ")")
        i += 1
        if depth == 0:
            break
        if i >= len(code):
            raise SystemExit(f"ref_build: unbalanced parameter list of {name} in {where}")
    body = re.compile(r"\s*\{").match(code, i)
    if not body:
        raise SystemExit(f"ref_build: {name} in {where} is a declaration, not a definition")
    i, depth = body.end(), 1
    while depth:
        if i >= len(code):
            raise SystemExit(f"ref_build: unbalanced body of {name} in {where}")
        depth += (code[i] == "{") - (code[i] == "}")
        i += 1
    return text[start:i]


def cut_all(ref: str) -> dict:
    out = {}
    for ns, files in KERNELS.items():
        parts = []
        for rel, names in files:
            path = os.path.join(ref, rel)
            if not os.path.isfile(path):
                raise SystemExit(f"ref_build: {path} not found")
            with open(path, encoding="utf-8", errors="replace") as f:
                text = f.read()
            for name in names:
                parts.append(f"// ---- {name}, cut from {rel}\n" + cut_function(text, name, rel))
        out[ns] = "\n\n".join(parts) + "\n"
    return out


def _write_if_changed(path: str, text: str) -> None:
    try:
        with open(path, encoding="utf-8") as f:
            if f.read() == text:
                return
    except OSError:
        pass
    with open(path, "w", encoding="utf-8") as f:
        f.write(text)


def build(force: bool = False) -> bool:
    """Returns True when both libraries exist afterwards."""
    ref = reference_dir()
    if not os.path.isdir(ref):
        have = all(os.path.exists(lib_path(v)) for v in VARIANTS)
        print(f"ref_build: no reference tree at {ref}; "
              f"{'keeping the existing' if have else 'there are no'} libraries under {OUT}")
        return have
    os.makedirs(OUT, exist_ok=True)
    incs = []
    for ns, text in cut_all(ref).items():
        inc = os.path.join(OUT, ns + ".inc")
        _write_if_changed(inc, text)
        incs.append(inc)
    deps = incs + [os.path.join(HERE, f) for f in ("ref_driver.cpp", "ref_shim.h", "ref_build.py")]
    cxx = os.environ.get("CXX", "g++")
    for variant, contract in VARIANTS.items():
        lib = lib_path(variant)
        if not force and os.path.exists(lib) and all(
                os.path.getmtime(lib) >= os.path.getmtime(d) for d in deps):
            continue
        tmp = lib + ".tmp"
        subprocess.run([cxx, *BASE_FLAGS, contract, "-I", OUT, "-I", HERE, "-o", tmp,
                        os.path.join(HERE, "ref_driver.cpp")], check=True)
        os.replace(tmp, lib)
    return True


if __name__ == "__main__":
    build(force="--force" in sys.argv[1:])
