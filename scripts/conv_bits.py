"""Bit-level record of the convolution entry points, for comparing two builds of the library (MDCTGAN_HIP_LIB picks one).

    python scripts/conv_bits.py OUT.json          # on a GPU: run every case, write one sha256 per output tensor
    python scripts/conv_bits.py --compare A.json B.json

Cases: every case of tests/test_conv_plan_coverage_host.walk_cases() with its planner hooks (forward with bias, data gradient,
weight gradient without and with the bias gradient, accumulate 0 and 1) and the no-workspace and unaligned rungs of
tests/test_conv_plans_gpu.test_entry_point_fallback_ladder, all inputs from one seed.  Equal digests are equal bits, which is
more than torch.equal asks (it would let -0.0 pass for 0.0)."""
import hashlib
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:32]


def set_env(keys, env):
    for k in keys:
        os.environ.pop(k, None)
    os.environ.update(env)


def run(out_path):
    import torch
    import test_conv_plan_coverage_host as cov
    import test_conv_plans_gpu as P
    from mdctgan_amd import _lib, ops
    lib = _lib.load()
    dev = "cuda"
    gen = torch.Generator().manual_seed(20240607)
    rec = {}

    def inputs(shape, g):
        B, Ci, H, W, Co, k, s, p, reflect = shape
        mk = lambda *sz: torch.randn(*sz, generator=gen).to(dev)
        return mk(B, H, W, Ci), mk(Co, k, k, Ci) / (Ci * k * k) ** 0.5, mk(Co), mk(B, g.OH, g.OW, Co)

    seen = set()
    for shape, prec, env, passes in cov.walk_cases():
        key = "%s|f%d|%s|%s" % (",".join(str(int(v)) for v in shape), 16 if prec else 32,
                                ";".join("%s=%s" % kv for kv in sorted(env.items())), "".join(str(p) for p in passes))
        if key in seen:
            continue
        seen.add(key)
        set_env(P.ENV_KEYS, env)
        g = P.geom_of(shape, prec)
        B, Ci, H, W, Co, k, s, p, reflect = shape
        x, w, b, gy = inputs(shape, g)
        if 0 in passes:
            rec[key + "|fwd"] = digest(ops.conv_fwd(g, x, w, b))
        if 1 in passes:
            rec[key + "|dgrad"] = digest(ops.conv_dgrad(g, gy, w))
        if 2 in passes:
            dw = torch.zeros(Co, k, k, Ci, device=dev)
            ops.conv_wgrad(g, x, gy, dw)
            rec[key + "|wgrad"] = digest(dw)
            db = torch.zeros(Co, device=dev)
            ops.conv_wgrad(g, x, gy, dw, db)
            rec[key + "|wgrad_db.dw"], rec[key + "|wgrad_db.db"] = digest(dw), digest(db)
            ops.conv_wgrad(g, x, gy, dw, db, accumulate=True)
            rec[key + "|wgrad_acc.dw"], rec[key + "|wgrad_acc.db"] = digest(dw), digest(db)
            ops.conv_wgrad(g, x, gy, dw, accumulate=True)
            rec[key + "|wgrad_acc_nodb.dw"] = digest(dw)
    # the entry points' fallback ladder, through the C ABI: no workspace, and every tensor one float off 16-byte alignment
    st = _lib.stream()
    for family, prec, shape, env in P.LADDER_CASES:
        set_env(P.ENV_KEYS, env)
        g = P.geom_of(shape, prec)
        B, Ci, H, W, Co, k, s, p, reflect = shape
        tensors = inputs(shape, g)
        for way in ("no_workspace", "unaligned_pointers"):
            un = way == "unaligned_pointers"
            x, w, b, gy = (P.offset_copy(t, un)[1] for t in tensors)

            def ws(ps):
                if not un:
                    return None, None, 0
                need = P.workspace_bytes(ps, g)
                buf = torch.zeros(need + 16, dtype=torch.uint8, device=dev)
                return buf, buf.data_ptr(), need

            key = "ladder|%s|%s" % (family, way)
            y = P.offset_copy(B * g.OH * g.OW * Co, un, fill=0.0)[1]
            keep, wsp, size = ws(0)
            rc = lib.mg_conv_fwd(g, x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), _lib.ACT_NONE, wsp, size, st)
            rec[key + "|fwd"] = [rc, digest(y)]
            dx = P.offset_copy(B * H * W * Ci, un, fill=0.0)[1]
            keep, wsp, size = ws(1)
            rc = lib.mg_conv_dgrad(g, gy.data_ptr(), w.data_ptr(), None, dx.data_ptr(), _lib.ACT_NONE, wsp, size, st)
            rec[key + "|dgrad"] = [rc, digest(dx)]
            dw, db = P.offset_copy(Co * k * k * Ci, un, fill=0.0)[1], P.offset_copy(Co, un, fill=0.0)[1]
            keep, wsp, size = ws(2)
            for acc in (0, 1):
                rc = lib.mg_conv_wgrad(g, x.data_ptr(), gy.data_ptr(), dw.data_ptr(), db.data_ptr(), acc, wsp, size, st)
                rec[key + "|wgrad_acc%d" % acc] = [rc, digest(dw), digest(db)]
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump({"lib": _lib.LIB_PATH, "records": rec}, f, indent=0, sort_keys=True)
    print(len(rec), "records ->", out_path)


def compare(a_path, b_path):
    a, b = (json.load(open(p))["records"] for p in (a_path, b_path))
    count = lambda r: sum(len(v) - 1 if isinstance(v, list) else 1 for v in r.values())
    bad = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
    print("tensors compared: %d and %d, records that differ: %d" % (count(a), count(b), len(bad)))
    for k in bad[:20]:
        print("  ", k, a.get(k), b.get(k))
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    run(sys.argv[1])
