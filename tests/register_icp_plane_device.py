"""What the GPU tests of lcd_register_icp_plane share (tests/test_gpu_register_icp_plane.py and tests/test_gpu_register_icp_plane_shapes.py):
the model's results per pair, cached; a batch staged on the device with canary-filled outputs; both entries; the exact comparison."""
import numpy as np
import pytest

import register_icp_plane_inputs as I
import register_icp_plane_model as M

LCD_ERR_INVALID, LCD_ERR_UNSUPPORTED = 1, 5
INTS = ("status", "stop", "iterations", "n_correspondences", "branch")
FLOATS = ("transform", "icp_transform", "correction", "ratio", "complexity", "complexity_values", "complexity_vectors", "second_eigenvalue")
PER_PAIR = INTS + FLOATS + ("variance",)
SEARCHES = (M.SEARCH_AUTO, M.SEARCH_BRUTE, M.SEARCH_GRID)
_model_cache = {}


def model_of(pair, **kw):
    key = (id(pair), tuple(sorted(kw.items())))
    if key not in _model_cache:
        _model_cache[key] = (pair, M.register(*I.scans(pair), **kw))       # the pair is kept so that its id stays its own
    return _model_cache[key][1]


def expected(pairs, device_entry=False, **kw):
    rs = [model_of(p, device_entry=device_entry, **kw) for p in pairs]
    out = {k: np.stack([np.asarray(r[k]) for r in rs]) for k in PER_PAIR}
    out["match"] = np.concatenate([r["match"] for r in rs] + [np.zeros(0, np.int32)])
    return out


def assert_same(got, want, what=""):
    for k in INTS + ("match",):
        np.testing.assert_array_equal(got[k], want[k], err_msg="%s %s" % (what, k))
    for k in FLOATS:
        np.testing.assert_array_equal(I.bits(got[k]).reshape(-1), I.bits(want[k]).reshape(-1), err_msg="%s %s" % (what, k))
    np.testing.assert_array_equal(np.ascontiguousarray(got["variance"]).view(np.uint64), np.ascontiguousarray(want["variance"], np.float64).view(np.uint64),
                                  err_msg=what + " variance")


def outputs_dev(n_pairs, n_from):
    """canary-filled output tensors of a call over n_pairs pairs and n_from from-rows"""
    import torch
    from rtabmap_amd import capi
    out = {}
    for k, w, dt in capi.Engine.ICP_PLANE_OUT:
        tdt = {np.int32: torch.int32, np.float32: torch.float32, np.float64: torch.float64}[dt]
        out[k] = torch.full((n_pairs, w) if w else (n_pairs,), -7 if dt is np.int32 else float("nan"), dtype=tdt, device="cuda")
    out["match"] = torch.full((max(n_from, 1),), -7, dtype=torch.int32, device="cuda")
    return out


def stage_dev(pairs):
    """the batch on the device, outputs canary-filled, uploaded and synchronised"""
    import torch
    fx, fn, fo, tx, tn, to, gs = I.concatenate(pairs)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    st = dict(fx=dev(fx), fn=dev(fn), fo=fo, tx=dev(tx), tn=dev(tn), to=to, gs=gs, out=outputs_dev(len(pairs), fx.shape[0]))
    torch.cuda.synchronize()
    return st


def launch_dev(eng, st, **kw):
    eng.register_icp_plane_dev(st["fx"], st["fn"], st["fo"], st["tx"], st["tn"], st["to"], st["gs"], st["out"], **kw)
    return st


def to_host(eng, st):
    eng.synchronize()
    out = {k: v.cpu().numpy() for k, v in st["out"].items()}
    out["match"] = out["match"][:int(st["fo"][-1])]
    return out


def run_dev(eng, pairs, **kw):
    return to_host(eng, launch_dev(eng, stage_dev(pairs), **kw))


def run_host(eng, pairs, **kw):
    fx, fn, fo, tx, tn, to, gs = I.concatenate(pairs)
    return eng.register_icp_plane(fx, fn, fo, tx, tn, to, gs, **kw)


def check_both(eng, pairs, what="", searches=(M.SEARCH_AUTO,), **kw):
    want = expected(pairs, **kw)
    for search in searches:
        assert_same(run_dev(eng, pairs, search=search, **kw), want, "%s dev, search %d" % (what, search))
        assert_same(run_host(eng, pairs, search=search, **kw), want, "%s host, search %d" % (what, search))
    return want


def refused(status, call, *args, **kw):
    from rtabmap_amd import capi
    with pytest.raises(capi.LcdError) as err:
        call(*args, **kw)
    assert err.value.status == status, err.value
