"""CPU checks of what tests/test_gpu_multiclass.py stands on: the oracle's refinement of a match the caller names
(oracle_py.refine_match, recognition_banks) against its own Recognition() where both apply -- one class --, the three-class
fixture (tests/multiclass.py, whose build() asserts the facts that keep the GPU tests from being vacuous), and the YAML
writer with more than one class."""
import ctypes as C
import os

import numpy as np
import pytest

import clutter
import multiclass
from test_abi_cpu import _cad, write_linemod_yaml

PARAMS = ((75.0, 10, 0.5, 0.01), (75.0, 20, 0.0, -3.0e38))
K16 = 16


@pytest.fixture(scope="module")
def mc(oracle):
    return multiclass.build(oracle)


def _same(a, e, tag):
    """Every field of result dict e is in a with the same bits."""
    for k, v in e.items():
        if isinstance(v, dict):
            _same(a[k], v, tag + (k,))
        elif isinstance(v, np.ndarray) or isinstance(v, np.floating):
            assert np.asarray(a[k]).dtype == np.asarray(v).dtype and np.asarray(a[k]).tobytes() == np.asarray(v).tobytes(), tag + (k,)
        else:
            assert a[k] == v, tag + (k,)


def test_one_bank_equals_recognition_and_topk(oracle, mc):
    """For one class the named-match path must be Recognition() itself: field for field on frames a and b, matches[0] and
    the first 16."""
    bank, K = mc["scene"]["bank"], mc["K"]
    for fi, f in ((0, "a"), (1, "b")):
        b, d = mc["bgrs"][fi], mc["depths"][fi]
        for p in PARAMS:
            exp = oracle.recognition(b, d, K, clutter.T, bank, *p)
            got = oracle.recognition_banks(b, d, K, clutter.T, [bank], 1, *p)
            assert exp["found"] == 1 and len(got) == 1 and got[0]["no_render"] is False
            _same(got[0], exp, (f, p))
        p = PARAMS[0]
        top, win = oracle.recognition_topk(b, d, K, clutter.T, bank, K16, *p, nms_dist=60.0)
        got, gwin = oracle.recognition_banks(b, d, K, clutter.T, [bank], K16, *p, nms_dist=60.0)
        assert len(top) == len(got) == K16 and gwin == win
        for r, (g, e) in enumerate(zip(got, top)):
            _same(g, e, (f, r))
        # and a single named match: the list's entry r with the list's length handed in
        m = oracle.match_images(b, d, clutter.T, [bank], p[0])[0]
        one = oracle.refine_match(d, K, bank, m[5], *p[1:], n_matches=len(m))
        _same(one, top[5], (f, "named"))


def test_class_filter_and_class_indices_of_recognition_banks(oracle, mc):
    """class_idx counts in the full sorted list whatever the filter and whatever the order the banks come in; a filter that
    names no class present matches nothing; a pyramid without a render is reported, not refined against an empty image."""
    K, b, d = mc["K"], mc["bgrs"][0], mc["depths"][0]
    full = oracle.recognition_banks(b, d, K, clutter.T, mc["added"], 12)
    assert [r["best"]["class_idx"] for r in full] == [int(c) for c in mc["lists"][0]["class_idx"][:12]]
    assert full[0]["n_matches"] == len(mc["lists"][0])
    for ids, idx in ((("mid",), 1), (("zeta", "nope"), 2), (("alpha",), 0)):
        got = oracle.recognition_banks(b, d, K, clutter.T, mc["added"], 4, class_ids=ids)
        # the class's own list (std::unique may keep fewer of a class's matches there than in the list over all classes, whose
        # repeats other classes' matches separate: the filtered list is not the global one with the other classes struck out)
        own, n_own = oracle.match_images(b, d, clutter.T, [mc["banks"][idx]], 75.0)
        assert len(got) == 4 and got[0]["n_matches"] == n_own <= int((mc["lists"][0]["class_idx"] == idx).sum())
        for g, m in zip(got, own):
            assert g["best"]["class_idx"] == idx and (g["best"]["x"], g["best"]["y"], g["best"]["template_id"]) == (m["x"], m["y"], m["template_id"])
            # the refinement of a match depends on the match alone, not on the list it came from
            named = dict(zip(m.dtype.names, m.tolist()), class_idx=idx)
            _same(g, dict(oracle.refine_match(d, K, mc["banks"][idx], named), n_matches=n_own), (ids,))
    assert oracle.recognition_banks(b, d, K, clutter.T, mc["added"], 4, class_ids=("nope",)) == []
    m = mc["lists"][0][1].copy()                      # a mid match, renamed to one of mid's random pyramids
    assert m["class_idx"] == 1
    m["template_id"] = 8 + 5
    r = oracle.refine_match(d, K, mc["by_id"]["mid"], m)
    assert r["no_render"] is True and r["found"] == 0 and r["best"]["template_id"] == 13
    with pytest.raises(IndexError):
        m["template_id"] = 108
        oracle.refine_match(d, K, mc["by_id"]["mid"], m)


def test_yaml_writer_with_two_classes(tmp_path, mc):
    """write_linemod_yaml with a list of banks: the reader finds both classes, in a file whose first class sorts last."""
    lib = _cad()
    p = str(tmp_path / "linemod_templates.yml")
    zeta, alpha = mc["by_id"]["zeta"], mc["by_id"]["alpha"]
    write_linemod_yaml(p, [zeta, alpha], clutter.T)
    lv, nc, nt, nf = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    assert lib.cadreco_read_linemod(p.encode(), C.byref(lv), C.byref(nc), C.byref(nt), C.byref(nf)) == 0
    assert (lv.value, nc.value, nt.value) == (2, 2, 16)
    nf2 = nf.value
    write_linemod_yaml(p, zeta, clutter.T)            # one bank, as every earlier caller passes it
    os.utime(p, (1, 1))
    assert lib.cadreco_read_linemod(p.encode(), C.byref(lv), C.byref(nc), C.byref(nt), C.byref(nf)) == 0
    assert (lv.value, nc.value, nt.value) == (2, 1, 8) and 0 < nf.value < nf2
