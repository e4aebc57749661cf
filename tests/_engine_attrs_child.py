"""Child of tests/test_gpu_engine_attrs.py: builds each of the six engine classes once, at the smallest shapes, in ONE fresh
process and writes what a caller can see of it: every public plain attribute, and what render hands back for each
want_u8 / want_pred combination (the parent compares the JSON with tests/golden/engine_attrs.json)."""
import json

import torch

from _gpu_child import child_main

PLAIN = (int, float, bool, str)
WANTS = [(True, False), (False, True), (True, True), (False, False)]       # (want_u8, want_pred); the last is illegal


def plain(v):
    return isinstance(v, PLAIN) or (isinstance(v, tuple) and all(isinstance(x, PLAIN) for x in v))


def attrs(eng):
    """every public non-callable attribute (properties included) that is an int, float, bool, str or a tuple of those; an
    attribute whose read raises is recorded by the exception's type"""
    out = {}
    for name in sorted(n for n in dir(eng) if not n.startswith("_")):
        try:
            v = getattr(eng, name)
        except Exception as e:
            out[name] = {"raises": type(e).__name__}
            continue
        if not callable(v) and plain(v):
            out[name] = v
    return out


def describe(t):
    return None if t is None else {"shape": list(t.shape), "dtype": str(t.dtype), "device": t.device.type}


def renders(call):
    """call(want_u8, want_pred) for the four combinations: shapes and dtypes, or the exception's type and text"""
    out = {}
    for u8, pred in WANTS:
        key = f"u8={int(u8)},pred={int(pred)}"
        try:
            a, b = call(u8, pred)
            out[key] = {"u8": describe(a), "pred": describe(b)}
        except Exception as e:
            out[key] = {"raises": type(e).__name__, "message": str(e)}
    torch.cuda.synchronize()
    return out


def rand(n, seed):
    return (0.05 * torch.randn(n, generator=torch.Generator().manual_seed(seed))).cuda()


def siren_like(eng):
    eng.set_coords(torch.linspace(0, 1, eng.height).cuda(), torch.linspace(0, 1, eng.width).cuda())
    eng.set_params(rand(eng.num_params, 1))
    if hasattr(eng, "set_encoding"):
        eng.set_encoding(rand(2 * (eng.map_size // 2), 2).reshape(2, -1).contiguous())
    return {"render": renders(lambda u, p: eng.render(want_u8=u, want_pred=p))}


def wavelet_like(eng):
    lin = torch.linspace(0, 1, eng.n).cuda()
    eng.set_coords(lin, lin)
    eng.set_params(rand(eng.num_params, 1))
    rows = getattr(eng, "max_rows", eng.height)                # the window a render handle was sized for
    out = {"render": renders(lambda u, p: eng.render(want_u8=u, want_pred=p))}
    if hasattr(eng, "max_rows"):
        out["render(0, max_rows)"] = renders(lambda u, p: eng.render(0, rows, want_u8=u, want_pred=p))
    else:
        out["render_window(0, H, 0, H)"] = renders(lambda u, p: eng.render_window(0, rows, 0, eng.height, u, p))
    return out


def cases():
    from implicit_image import _engine as E
    return [("SirenEngine", lambda: E.SirenEngine(8, 12, 64, 3, row_begin=2, row_end=6), siren_like),
            ("RenderEngine", lambda: E.RenderEngine(8, 12, 64, 3), siren_like),
            ("FourierEngine", lambda: E.FourierEngine(8, 12, 64, 3, 64), siren_like),
            ("FourierRenderEngine", lambda: E.FourierRenderEngine(8, 12, 64, 3, 64), siren_like),
            ("WaveletEngine", lambda: E.WaveletEngine(30, 30, 64, 3), wavelet_like),
            ("WaveletRenderEngine", lambda: E.WaveletRenderEngine(30, 64, 3, max_rows=7), wavelet_like)]


def case_engine_attrs():
    torch.cuda.init()
    res = {}
    for name, make, use in cases():
        eng = make()
        rec = {"class": type(eng).__name__, "bases": [c.__name__ for c in type(eng).__mro__[1:-1]], "attrs": attrs(eng)}
        rec.update(use(eng))
        eng.close()
        res[name] = rec
        print(name, json.dumps(rec["attrs"]), flush=True)
    return res


if __name__ == "__main__":
    child_main({"engine_attrs": case_engine_attrs})
