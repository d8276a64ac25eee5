"""
Host side of the device-resident two-stage blind phase search (``method="fused"``): argument checks, the C ABI's three
descriptions of the new entry points, and the table of fine-angle offsets.  No GPU needed.
"""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, RT, golden_cases
from qampy_amd import _lib
from qampy_amd.core import hip_dsp, phaserecovery as core_ph

NAMES = ("qh_bps_twostage_recover_c64_dev", "qh_bps_twostage_recover_c128_dev")


def test_fused_is_a_known_method_and_others_are_still_rejected(monkeypatch):
    seen = {}

    def fake(E, Mtestangles, symbols, N, B=4):
        seen.update(shape=E.shape, A=Mtestangles, N=N, B=B, sdt=symbols.dtype)
        return E * 1, np.zeros(E.shape, E.real.dtype)

    monkeypatch.setattr(core_ph._dsp, "bps_twostage_recover", fake)
    E = np.ones(32, np.complex64)
    out, ph = core_ph.bps_twostage(E, 8, np.ones(4, np.complex128), 4, B=6, method="fused")
    assert out.shape == ph.shape == (32,) and ph.dtype == np.float32              # 1-d in, 1-d out
    assert seen == dict(shape=(1, 32), A=8, N=4, B=6, sdt=np.dtype(np.complex64))   # one call for all rows, alphabet in the signal's dtype
    out, ph = core_ph.bps_twostage(np.ones((3, 32), np.complex128), 8, np.ones(4, np.complex128), 4, method="FUSED")
    assert out.shape == ph.shape == (3, 32) and seen["shape"] == (3, 32) and seen["B"] == 4
    for bad in ("af", "pyx", "fuse"):
        with pytest.raises(ValueError):
            core_ph.bps_twostage(E, 8, np.ones(4, np.complex64), 4, method=bad)


def test_fused_keeps_the_signal_subclass(monkeypatch):
    from qampy_amd.signals import SignalQAM
    monkeypatch.setattr(core_ph._dsp, "bps_twostage_recover", lambda E, A, s, N, B=4: (E * 1, np.zeros(E.shape, E.real.dtype)))
    import qampy_amd
    sig = SignalQAM(np.ones((2, 16), np.complex64), 4)
    out, ph = qampy_amd.phaserec.bps_twostage(sig, 8, 4, B=2, method="fused")
    assert type(out) is SignalQAM and out.M == 4 and out.shape == (2, 16) and type(ph) is np.ndarray


def test_wrapper_rejects_what_is_not_a_2d_complex_array_before_touching_the_device():
    with pytest.raises(TypeError):
        hip_dsp.bps_twostage_recover(np.zeros((2, 64), np.float32), 8, np.ones(4, np.complex64), 4)
    with pytest.raises(TypeError):
        hip_dsp.bps_twostage_recover(np.zeros(64, np.complex64), 8, np.ones(4, np.complex64), 4)
    with pytest.raises(TypeError):
        hip_dsp.bps_twostage_recover(np.zeros((2, 64), np.complex64), 8, np.ones(4, np.complex128), 4)
    out, ph = hip_dsp.bps_twostage_recover(np.zeros((2, 0), np.complex64), 8, np.ones(4, np.complex64), 4)      # L == 0: empties, no device
    assert out.shape == ph.shape == (2, 0) and out.dtype == np.complex64 and ph.dtype == np.float32


def test_header_signature_table_and_entry_points_agree():
    header = open(os.path.join(ROOT, "include", "qampy_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    api = open(os.path.join(ROOT, "qampy_amd", "csrc", "api.hip")).read()
    lib = _lib.load()
    for n in NAMES:
        decl = re.search(r"int %s\s*\((.*?)\);" % n, header, flags=re.S)
        assert decl, "%s is not declared in include/qampy_hip.h" % n
        params = [p.strip() for p in decl.group(1).split(",")]
        assert [p.split()[-1].lstrip("*") for p in params] == ["E", "nm", "L", "angles", "A", "B", "symbols", "M", "N", "idx1", "idx2", "ph", "Eout"]
        assert n in _lib.SIGNATURES and len(_lib.SIGNATURES[n]) == len(params)
        import ctypes as C
        want = [C.c_int64 if p.startswith("int64_t") else (C.c_int if p.startswith("int ") else C.c_void_p) for p in params]
        assert _lib.SIGNATURES[n] == want
        defn = re.search(r"^int %s\s*\((.*?)\)\s*\{" % n, api, flags=re.S | re.M)
        assert defn, "%s is not defined in csrc/api.hip" % n
        assert re.sub(r"\s+", " ", defn.group(1)) == re.sub(r"\s+", " ", decl.group(1))
        assert hasattr(lib, n)
    assert _lib.ABI_VERSION == 11 == lib.qh_abi_version()              # additive: the version stays


@pytest.mark.parametrize("rt", [np.float32, np.float64])
@pytest.mark.parametrize("A,B", [(8, 1), (8, 2), (16, 4), (32, 6), (8, 6), (64, 64), (16, 5)])
def test_offsets_reproduce_the_reference_fine_grid_bit_for_bit(A, B, rt):
    """What the fused path adds to a coarse angle, against the expression of core/phaserecovery.py:51 evaluated for every coarse angle."""
    coarse = hip_dsp.test_angle_grid(A, rt)
    off = hip_dsp.twostage_offsets(A, B)
    assert off.dtype == np.float64 and off.shape == (B,)
    table = (coarse[0].astype(np.float64)[:, np.newaxis] + off[np.newaxis, :]).astype(rt)
    first = coarse[0]                                                   # select_angles of every index once
    steps = np.linspace(-B / 2, B / 2, B)
    fine = (first[:, np.newaxis] + steps[np.newaxis, :] / (B * A) * np.pi / 2).astype(rt)
    assert fine.dtype == table.dtype and np.array_equal(fine, table)
    if B > 1:                                                           # the grid spans one coarse step around the estimate, ends included
        assert off[0] == -off[-1] == -np.pi / 4 / A


@pytest.mark.parametrize("case", golden_cases("twostage"), ids=lambda c: c["name"])
def test_offsets_against_the_golden_phases(golden, case):
    """The stored ``ph`` is the unwrapped track, and every interior sample carries a wrap: only the first ``N`` samples of a row - index 0 in both
    stages, in front of the first wrap - hold a fine-grid value as it was selected.  Those are compared bit for bit; every other sample must be
    a table value up to the wrap it carries."""
    rt = RT[case["dtype"]]
    A, B, N = case["A"], case["B"], case["N"]
    table = (hip_dsp.test_angle_grid(A, rt)[0].astype(np.float64)[:, np.newaxis] + hip_dsp.twostage_offsets(A, B)[np.newaxis, :]).astype(rt)
    ph = golden["twostage"][case["name"] + "__ph"]
    assert ph.dtype == rt and np.all(ph[:, :N] == table[0, 0])
    wraps = np.round((ph[..., np.newaxis] - table.reshape(-1)) / (np.pi / 2))
    resid = np.abs(ph[..., np.newaxis] - table.reshape(-1) - wraps * (np.pi / 2)).min(axis=-1)
    assert resid.max() < (1e-12 if rt is np.float64 else 1e-6)
