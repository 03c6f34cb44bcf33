#!/usr/bin/env python3
"""What the library's host side answers about convolution launches -- which kernel and configuration a descriptor resolves to, the
candidate list, the slab rows -- for a fixed table of descriptors, every element type and every candidate configuration.

usage: tools/conv_plan_dump.py [--write]
  prints one line per (descriptor, type); --write records everything in GOLDEN, the fixture of tests/test_conv_plan_host.py.

The fixture characterises the resolver: it was recorded from the library BEFORE the host layer of the forward / data-gradient convolution
was split by role, and is not regenerated when that layer is refactored -- only when the tile tables or the default choice change on
purpose.  Host arithmetic only: no GPU.  Rows of pointwise configurations are left out (None): they come from an occupancy query that
answers differently with and without a device."""
import ctypes as C
import json
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_plan.json")
DTYPES = {"bf16": 1, "fp16": 2, "fp32": 0}          # LH_BF16, LH_F16, LH_F32
FIELDS = ["cfg0", "cfg1", "cfg2", "cfg3", "config_rc", "out0", "out1", "out2", "out3", "out4", "tile_rc", "bm", "bp", "ring",
          "stats_rows", "gated_rows_1", "gated_rows_2"]
MAXC = 128
N = 2                                               # batch: a host table, no work is done


def _taps(k):
    return [(r - k // 2, s - k // 2) for r in range(k) for s in range(k)]


def _conv(cin, cout, h, w, k, s=1, k_run=None):
    from lighthand_amd.graph import _desc
    p = (k - 1) // 2
    ho, wo = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
    return _desc(N, h, w, k_run or cin, k_run or cin, ho, wo, s, s, cout, ho, wo, 1, 1, 0, 0, cout, _taps(k))


def _dgrad(cin, cout, h, w, k):
    """Data gradient of a stride-1 k x k convolution cin -> cout: the mirrored taps, channels swapped."""
    from lighthand_amd.graph import _desc
    return _desc(N, h, w, cout, cout, h, w, 1, 1, cin, h, w, 1, 1, 0, 0, cin, [(-a, -b) for a, b in _taps(k)])


def _phases(cin, cout, h, w, rows):
    """Four sub-pixel phases on an h x w input that fill a 2h x 2w output; rows[parity] = the tap offsets of that parity."""
    from lighthand_amd.graph import _desc
    return [_desc(N, h, w, cin, cin, h, w, 1, 1, cout, 2 * h, 2 * w, 2, 2, ph, pw, cout, [(a, b) for a in rows[ph] for b in rows[pw]])
            for ph in range(2) for pw in range(2)]


def descriptors():
    """name -> descriptor; the members of a phase set are named '<set>.<i>' (phase_sets())."""
    from lighthand_amd.graph import _desc
    d = {
        "1x1 64->256 64x64": _conv(64, 256, 64, 64, 1),
        "1x1 256->64 64x64": _conv(256, 64, 64, 64, 1),
        "1x1 520->64 16x16": _conv(520, 64, 16, 16, 1),                 # K run too wide for the pointwise kernel
        "3x3 64->64 32x32": _conv(64, 64, 32, 32, 3),                   # the direct kernel
        "3x3 40->72 13x11": _conv(40, 72, 13, 11, 3),
        "3x3 256->256 16x16": _conv(256, 256, 16, 16, 3),
        "3x3s2 128->128 32x32": _conv(128, 128, 32, 32, 3, 2),
        "dgrad 3x3 64->64 32x32": _dgrad(64, 64, 32, 32, 3),
        "dgrad 3x3 40->72 13x11": _dgrad(40, 72, 13, 11, 3),
        "dgrad 3x3 256->256 16x16": _dgrad(256, 256, 16, 16, 3),
        "3x3 256->128 16x16": _conv(256, 128, 16, 16, 3),               # one 128-row block in the pack: no 256-row tile
        # irregular tap list: lh_tap_grid refuses it, the launch resolves to the register-staged kernel
        "plus 40->72 13x11": _desc(N, 13, 11, 40, 40, 13, 11, 1, 1, 72, 13, 11, 1, 1, 0, 0, 72, [(-1, 0), (0, -1), (0, 0), (0, 1), (1, 0)]),
    }
    # the data gradient of the 3x3 / stride 2 (1, 2, 2 and 4 taps) and the 4x4 / stride 2 transposed convolution (2 x 2 taps each)
    for name, phases in (("dgrad 3x3s2 128->128 16x16", _phases(128, 128, 16, 16, ((0,), (1, 0)))),
                         ("deconv 4x4s2 256->256 16x16", _phases(256, 256, 16, 16, ((0, -1), (1, 0))))):
        for i, p in enumerate(phases):
            d[f"{name}.{i}"] = p
    return d


PHASE_SETS = ["dgrad 3x3s2 128->128 16x16", "deconv 4x4s2 256->256 16x16"]
# (descriptor, type, explicit cfg, substring of lh_last_error()): configurations the library refuses
REFUSALS = [
    ("3x3 256->128 16x16", "bf16", (256, 256, 3, 64), "does not fit"),
    ("3x3 256->128 16x16", "bf16", (128, 128, 32, 128), "not compiled in"),
    ("3x3 256->128 16x16", "bf16", (128, 128, 12, 128), "not compiled in"),       # the removed wide-wave codes 10..19
    ("3x3 256->128 16x16", "fp16", (128, 128, 55, 64), "not compiled in"),        # 30..99
    ("3x3 256->128 16x16", "bf16", (128, 16, 1, 256), "pointwise configuration"),  # not a 1x1 form
    ("1x1 256->64 64x64", "bf16", (256, 16, 1, 512), "pointwise configuration"),   # wrong K padding
    ("1x1 256->64 64x64", "fp32", (128, 16, 1, 256), "pointwise configuration"),   # 16-bit types only
    ("1x1 520->64 16x16", "bf16", (64, 16, 1, 512), "pointwise configuration"),
    ("3x3 40->72 13x11", "bf16", (64, 256, 100, 40), "direct 3x3 configuration"),
    ("3x3 64->64 32x32", "fp32", (64, 256, 100, 64), "direct 3x3 configuration"),
    ("3x3 64->64 32x32", "fp32", (128, 128, 22, 128), "not compiled in"),          # dense-wave forms: 16-bit types only
]


def set_cfg(d, cfg):
    for j in range(8):
        d.cfg[j] = 0
    for j, v in enumerate(cfg):
        d.cfg[j] = v


def record(lib, d, dt, cfg):
    """One row of FIELDS for descriptor d with the explicit configuration cfg ((0, 0, 0, 0): the library's default)."""
    set_cfg(d, cfg)
    out = (C.c_int * 5)(-9, -9, -9, -9, -9)
    bm, bp, ring = C.c_int(-9), C.c_int(-9), C.c_int(-9)
    rc = lib.lh_igemm_config(C.byref(d), dt, out)
    trc = lib.lh_igemm_tile(C.byref(d), dt, C.byref(bm), C.byref(bp), C.byref(ring))
    rows = [lib.lh_igemm_stats_rows(C.byref(d), dt), lib.lh_igemm_gated_rows(C.byref(d), dt, 1), lib.lh_igemm_gated_rows(C.byref(d), dt, 2)]
    if rc == 0 and out[2] == 1:                     # pointwise: the occupancy query's answer is not the fixture's business
        rows = [None, None, None]
    set_cfg(d, (0, 0, 0, 0))
    return list(cfg) + [rc] + list(out) + [trc, bm.value, bp.value, ring.value] + rows


def candidates(lib, d, dt):
    buf = (C.c_int * (5 * MAXC))()
    set_cfg(d, (0, 0, 0, 0))
    n = lib.lh_igemm_candidates(C.byref(d), dt, buf, MAXC)
    assert 0 <= n < MAXC
    flat = list(buf[:5 * n])
    return [tuple(flat[5 * i:5 * i + 4]) for i in range(n)], zlib.crc32(",".join(map(str, flat)).encode())


def dump(lib):
    os.environ.pop("LH_DENSE_TILES", None)
    descs = descriptors()
    cases, phases, refusals = {}, {}, []
    for name, d in descs.items():
        for tname, dt in DTYPES.items():
            cands, crc = candidates(lib, d, dt)
            cases[f"{name} {tname}"] = {"candidates": [len(cands), crc], "rows": [record(lib, d, dt, c) for c in [(0, 0, 0, 0)] + cands]}
    for name in PHASE_SETS:
        ds = [descs[f"{name}.{i}"] for i in range(4)]
        arr = (C.POINTER(type(ds[0])) * 4)(*[C.pointer(x) for x in ds])
        lead = max(range(4), key=lambda i: (ds[i].ntaps, -i))
        for tname, dt in DTYPES.items():
            got = []
            for c in [(0, 0, 0, 0)] + candidates(lib, ds[lead], dt)[0]:
                set_cfg(ds[lead], c)
                got.append(lib.lh_igemm_phases_rows(arr, 4, dt))
            set_cfg(ds[lead], (0, 0, 0, 0))
            phases[f"{name} {tname}"] = got
    for name, tname, cfg, text in REFUSALS:
        row = record(lib, descs[name], DTYPES[tname], cfg)
        set_cfg(descs[name], cfg)
        lib.lh_igemm_config(C.byref(descs[name]), DTYPES[tname], (C.c_int * 5)())
        said = text.encode() in lib.lh_last_error()
        set_cfg(descs[name], (0, 0, 0, 0))
        refusals.append([name, tname, text, said] + row)
    return {"fields": FIELDS, "cases": cases, "phases_rows": phases, "refusals": refusals}


def main():
    from lighthand_amd import _lib
    got = dump(_lib.load())
    for case, v in got["cases"].items():
        print(f"{case:40s} {v['candidates'][0]:3d} candidates, default {v['rows'][0][5:10]}, rows {v['rows'][0][14:]}")
    for r in got["refusals"]:
        print("refusal", r[:4], r[4:9])
    if "--write" in sys.argv[1:]:
        assert all(r[3] and r[8] != 0 for r in got["refusals"]), "a configuration of REFUSALS was accepted, or refused in other words"
        with open(GOLDEN, "w") as f:
            parts = []
            for k, v in got.items():
                if k == "cases":
                    body = ",\n".join(f"    {json.dumps(c)}: {{\"candidates\": {json.dumps(e['candidates'])}, \"rows\": [\n      "
                                      + ",\n      ".join(json.dumps(r) for r in e["rows"]) + "]}" for c, e in v.items())
                    parts.append(f"  \"cases\": {{\n{body}\n  }}")
                elif k == "refusals":
                    parts.append("  \"refusals\": [\n    " + ",\n    ".join(json.dumps(r) for r in v) + "]")
                else:
                    parts.append(f"  {json.dumps(k)}: {json.dumps(v)}")
            f.write("{\n" + ",\n".join(parts) + "\n}\n")
        print(f"{len(got['cases'])} cases -> {GOLDEN} ({os.path.getsize(GOLDEN)} bytes)")


if __name__ == "__main__":
    main()
