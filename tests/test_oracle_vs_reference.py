# coding=utf-8
"""Pins the oracle to the REFERENCE'S OWN PYTHON.

* ``test_oracle_matches_reference_golden``: oracle/tfg_oracle.py vs tests/golden/reference_cases.npz — the outputs the
  unmodified /root/reference/tf_geometric produced (tests/golden/make_golden_from_reference.py).  Runs anywhere.
* ``test_golden_file_is_what_the_reference_produces`` / ``test_oracle_equals_reference_python`` and the other checks
  below: where the reference checkout exists they re-run the reference live — the committed files must be reproduced
  bit for bit, and on further fuzz seeds the oracle must agree with the live reference.  Elsewhere they run against
  tests/golden/reference_checks.npz (what the live reference returned, written with the golden vectors): the inputs
  the golden vectors were computed from, the fuzz outputs, the split-size table, the harness on a stand-in package.
No GPU, no product code: this file only relates the checker to the reference."""
import os
import types

import numpy as np
import pytest

from conftest import ROOT, assert_parity
import reference_cases as rc
from oracle.ref_harness import load_reference, reference_available

GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_cases.npz")


def compare(case, got, golden, who):
    keys = [k for k in golden if k.startswith(case.name + "::")]
    assert keys, "no golden entries for " + case.name
    for full in keys:
        k = full[len(case.name) + 2:]
        if k not in got:
            if "::" in k:        # layer weights stored for the product executor
                continue
            raise AssertionError("{} did not produce {}::{}".format(who, case.name, k))
        a, b = np.asarray(got[k]), golden[full]
        assert a.shape == b.shape, "{}::{} shape {} vs reference {}".format(case.name, k, a.shape, b.shape)
        if k in case.exact:
            assert np.array_equal(a, b), "{}::{} must be bit-identical to the reference".format(case.name, k)
        else:
            assert_parity(a, b, tol=case.tol_of(k), what="{} {}::{}".format(who, case.name, k))


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


@pytest.mark.parametrize("case", [c for c in rc.CASES if c.orc is not None], ids=lambda c: c.name)
def test_oracle_matches_reference_golden(case, oracle, golden):
    compare(case, case.orc(oracle, case.inputs()), golden, "oracle")


CHECKS = os.path.join(ROOT, "tests", "golden", "reference_checks.npz")


@pytest.fixture(scope="module")
def checks():
    return dict(np.load(CHECKS))


@pytest.fixture(scope="module")
def R():
    """The reference, loaded unmodified, where its checkout exists; None elsewhere — the checks below then run against
    tests/golden/reference_checks.npz, which holds what the live reference returned for them."""
    if not reference_available():
        return None
    tfg, tf, tfs, backend = load_reference()
    return types.SimpleNamespace(tfg=tfg, tf=tf, tfs=tfs, backend=backend)


def test_reference_is_loaded_unmodified(R, checks, tmp_path):
    if R is not None:
        from oracle.ref_harness.load_reference import REFERENCE_ROOT
        rc.check_loaded_unmodified(R.tfg, REFERENCE_ROOT)
        import hashlib
        for rel in rc.REFERENCE_FILES:        # the reference version the stored checks were taken from
            with open(os.path.join(REFERENCE_ROOT, "tf_geometric", rel), "rb") as f:
                assert hashlib.sha1(f.read()).hexdigest() == str(checks["sha1::" + rel]), rel
        return
    # no checkout here: the harness, in a process of its own, on a stand-in package at $TFG_REFERENCE_ROOT
    import subprocess
    import sys
    for rel in ("__init__.py",) + tuple(os.path.join(os.path.dirname(r), "__init__.py") for r in rc.REFERENCE_FILES) + \
            rc.REFERENCE_FILES:
        path = tmp_path / "tf_geometric" / rel
        path.parent.mkdir(parents=True, exist_ok=True)
        if not path.exists():
            path.write_text("# stand-in for tf_geometric/{} (reference sha1 {})\n".format(
                rel, checks.get("sha1::" + rel, "-")))
    code = ("import sys; sys.path[:0] = [{!r}, {!r}]; import reference_cases as rc; "
            "from oracle.ref_harness import load_reference; tfg, tf, tfs, backend = load_reference(); "
            "rc.check_loaded_unmodified(tfg, {!r}); print('ok', backend)").format(ROOT, os.path.join(ROOT, "tests"),
                                                                                 str(tmp_path))
    res = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, TFG_REFERENCE_ROOT=str(tmp_path)),
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert res.returncode == 0 and res.stdout.decode().startswith("ok"), res.stderr.decode()[-3000:]


@pytest.mark.parametrize("case", rc.CASES, ids=lambda c: c.name)
def test_golden_file_is_what_the_reference_produces(case, R, golden, checks):
    inputs = case.inputs()
    # the committed vectors were computed from exactly these inputs (digest taken when they were written)
    assert rc.inputs_digest(inputs) == str(checks["inputs_sha256::" + case.name]), \
        "{}: inputs changed since tests/golden was written — regenerate".format(case.name)
    assert any(k.startswith(case.name + "::") for k in golden), case.name
    if R is None:
        return
    if str(golden["__backend__"]) != R.backend:
        pytest.skip("golden file was generated on backend {}".format(golden["__backend__"]))
    live = case.ref(R, inputs)
    for k, v in live.items():
        assert np.array_equal(np.asarray(v), golden["{}::{}".format(case.name, k)], equal_nan=True), \
            "{}::{}: committed golden differs from the live reference — regenerate".format(case.name, k)


@pytest.mark.parametrize("seed", rc.FUZZ_SEEDS)
def test_oracle_equals_reference_python(seed, R, oracle, checks):
    """Fuzz: fresh graphs (duplicates, self-loops, isolated nodes), hot-path functions, oracle vs the reference — live where
    it exists (and then also against its stored outputs), its stored outputs elsewhere."""
    p = rc.fuzz_check_inputs(seed)
    ref = {k[len("fuzz{}::".format(seed)):]: v for k, v in checks.items() if k.startswith("fuzz{}::".format(seed))}
    assert ref, "no stored outputs for fuzz seed {}".format(seed)
    if R is not None:
        live = rc.fuzz_check_ref(R, p)
        if R.backend == str(checks["__backend__"]):
            assert sorted(live) == sorted(ref)
            for k, v in live.items():
                assert np.array_equal(np.asarray(v), ref[k], equal_nan=True), "fuzz{}::{} differs from the stored".format(seed, k)
        ref = live
    got = rc.fuzz_check_orc(oracle, p)
    assert sorted(got) == sorted(ref)
    for k, v in got.items():
        if k == "aggregate-max":
            assert np.array_equal(v, np.asarray(ref[k])), k
        else:
            assert_parity(v, ref[k], what=k)


def test_num_splits_rule_equals_reference(R, checks):
    """dist.sharded.compute_num_or_size_splits (column-chunked halo) vs the reference's helper of the same name
    (utils/tf_sparse_utils.py:71-90): same split sizes, same refusals."""
    import json
    from tf_geometric_amd.dist.sharded import compute_num_or_size_splits as mine
    want = json.loads(str(checks["num_splits"]))
    if R is not None:
        assert rc.num_splits_table(R.tfg.utils.tf_sparse_utils.compute_num_or_size_splits) == want
    assert rc.num_splits_table(mine) == want


def test_the_one_widened_tolerance_is_inherent_to_fp32(oracle, golden):
    """Every golden comparison uses the plain band 1e-5 + 1e-5*|ref| except propagation_convs::chebynet-None (2e-4).
    Evidence that this widening is a property of fp32, not of the HIP path: the REFERENCE'S OWN fp32 output (the golden
    vector) is itself several bands away from the float64-accumulated value of the same formula, while on every other
    output of the case it sits well inside one band."""
    case = rc.by_name("propagation_convs")
    exact = case.orc(oracle, case.inputs())
    widened = [k for k in exact if case.tol_of(k) != rc.TOL]
    assert widened == ["chebynet-None"]
    for k, v in exact.items():
        ref32 = golden["propagation_convs::" + k].astype(np.float64)
        v = np.asarray(v, np.float64)
        ratio = float((np.abs(ref32 - v) / (1e-5 + 1e-5 * np.abs(v))).max())
        if k in widened:
            assert ratio > 3.0, (k, ratio)          # measured 9.1: the reference itself leaves the plain band
        else:
            assert ratio < 0.5, (k, ratio)
    assert all(c.tol == rc.TOL for c in rc.CASES)
    assert sum(len(c.key_tol) for c in rc.CASES) == 1
