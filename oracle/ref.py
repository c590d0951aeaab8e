"""ctypes/numpy wrapper over the reference's own kernels built for the host
(``oracle/_ref/libpp2_ref_{fma,nofma}.so``, made by ``ref_build.py``).

TEST INFRASTRUCTURE ONLY.  The functions mirror ``oracle.model_pomdp``,
``model_mdp``, ``mdp_sweep``, ``belief_update``, ``fib_sweep`` and
``pbvi_gamma_ao`` -- same arguments, same layouts, same results if the oracle
restates the kernels correctly -- with two more keywords:

``variant``  ``"fma"`` (default): a*b+c contracted to fma like the reference's
             nvcc build; ``"nofma"``: no contraction, the sensitivity control.
``ftz``      flush-to-zero and denormals-are-zero for the call (default on,
             the reference's device arithmetic); the caller's MXCSR is
             restored afterwards.

This module never builds anything and never reads the reference tree:
``available()`` says whether the libraries are there.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
VARIANTS = ("fma", "nofma")

_f32p = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")
_u8p = np.ctypeslib.ndpointer(np.uint8, flags="C_CONTIGUOUS")


def lib_path(variant: str = "fma") -> str:
    return os.path.join(HERE, "_ref", f"libpp2_ref_{variant}.so")


def available() -> bool:
    return all(os.path.exists(lib_path(v)) for v in VARIANTS)


_libs = {}


def lib(variant: str = "fma"):
    if variant not in VARIANTS:
        raise ValueError(f"unknown variant {variant!r}")
    if variant not in _libs:
        L = C.CDLL(lib_path(variant))
        I, F = C.c_int, C.c_float
        sig = {
            "ref_model_pomdp": (None, [I, I, _u8p, I, I, _f32p, _f32p, _f32p, I]),
            "ref_model_mdp": (None, [I, I, _u8p, I, I, _f32p, _f32p, I]),
            "ref_mdp_sweep": (None, [I, I, F, _f32p, _f32p, _f32p, _f32p, _u8p, I]),
            "ref_belief_update": (None, [I, I, _f32p, _f32p, _f32p, I, I, _f32p, I]),
            "ref_fib_sweep": (None, [I, I, F, _f32p, _f32p, _f32p, _f32p, _f32p, I]),
            "ref_gamma_ao": (None, [I, I, F, _f32p, _f32p, I, I, I, _f32p, _f32p, I]),
            "ref_mxcsr": (C.c_uint, []),
        }
        for name, (res, args) in sig.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _libs[variant] = L
    return _libs[variant]


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def model_pomdp(grid, goal, variant="fma", ftz=True):
    H, W = grid.shape
    T = np.zeros((H * W, 9, 9), np.float32)
    Lk = np.zeros((H * W, 16), np.float32)
    R = np.zeros((H * W, 9), np.float32)
    lib(variant).ref_model_pomdp(H, W, np.ascontiguousarray(grid, np.uint8), int(goal[0]),
                                 int(goal[1]), T, Lk, R, int(ftz))
    return T, Lk, R


def model_mdp(grid, goal, variant="fma", ftz=True):
    H, W = grid.shape
    T = np.zeros((H * W, 9, 9), np.float32)
    Cc = np.zeros((H * W, 9), np.float32)
    lib(variant).ref_model_mdp(H, W, np.ascontiguousarray(grid, np.uint8), int(goal[0]),
                               int(goal[1]), T, Cc, int(ftz))
    return T, Cc


def mdp_sweep(H, W, gamma, T, Cc, J, variant="fma", ftz=True):
    Jo = np.empty(H * W, np.float32)
    A = np.empty(H * W, np.uint8)
    lib(variant).ref_mdp_sweep(H, W, float(gamma), _f32(T), _f32(Cc), _f32(J), Jo, A, int(ftz))
    return Jo, A


def belief_update(H, W, T, L, b, u, z, ftz=True, variant="fma"):
    out = np.empty(H * W, np.float32)
    lib(variant).ref_belief_update(H, W, _f32(T), _f32(L), _f32(b), int(u), int(z), out, int(ftz))
    return out


def fib_sweep(H, W, gamma, T, L, R, a, variant="fma", ftz=True):
    out = np.empty((H * W, 9), np.float32)
    lib(variant).ref_fib_sweep(H, W, float(gamma), _f32(T), _f32(L), _f32(R), _f32(a), out,
                               int(ftz))
    return out


def pbvi_gamma_ao(H, W, gamma, T, L, a, o, alphas, variant="fma", ftz=True):
    """cudaComputeGammaOA for one (a, o): out[k, x] for alphas[k, x]."""
    alphas = _f32(alphas).reshape(-1, H * W)
    out = np.empty_like(alphas)
    lib(variant).ref_gamma_ao(H, W, float(gamma), _f32(T), _f32(L), int(a), int(o),
                              alphas.shape[0], alphas, out, int(ftz))
    return out


def mxcsr(variant="fma") -> int:
    """The calling thread's MXCSR (to check that a call left it unchanged)."""
    return int(lib(variant).ref_mxcsr())
