#!/usr/bin/env python3
"""One search call per launch path of the enqueue (islands_amd/csrc/search_launch_plan.hpp) and one prepare(), small
enough to take seconds: a few thousand rows, d = 40 and 768, 70 queries.  Meant to run under
`rocprofv3 --kernel-trace --output-format csv -d <dir> -- python tools/launch_trace.py --part main`, once per build;
`--compare A B` then sets two such traces' dispatches side by side (name, grid, workgroup, LDS), the way
profiles/launch_plan_trace_ab.json records.  Inputs are seeded, so two builds that launch the same see the same rows.
`--part recompute` makes the calls over the recompute provider, whose rounds are not the same twice even on one build:
their traces are compared with `--distinct`."""
import argparse
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))


def run(part):
    import numpy as np

    import bert_ref
    import islands_amd as ia

    rng = np.random.default_rng(7)
    nq, k = 70, 10

    def rows(n, d, seed):
        r = np.random.default_rng(seed)
        return (r.random((n, d), dtype=np.float32) * 2.0 - 1.0).astype(np.float32)

    def bf16_bits(a):
        return (np.ascontiguousarray(a).view(np.uint32) >> 16).astype(np.uint16)

    def widen(b):
        return (b.astype(np.uint32) << 16).view(np.float32)

    def csr(n, deg, seed):
        nb = np.random.default_rng(seed).integers(0, n, (n, deg)).astype(np.uint64)
        off = (np.arange(n + 1, dtype=np.uint64) * np.uint64(deg))
        return ia.CsrGraph(node_offsets=off, neighbors=nb.reshape(-1), levels=np.zeros(n, np.uint64), entry_point=0,
                           num_nodes=n, degree_counts=np.full(n, deg, np.uint64))

    def index(g, d, install):
        idx = ia.LeannIndex.from_csr(g, None, dimension=d).upload(0)
        install(idx)
        return idx

    def pq_of(v, m, K, seed):
        r = np.random.default_rng(seed)
        n, d = v.shape
        dsub = d // m
        cb = np.stack([v[r.choice(n, K, replace=False), j * dsub:(j + 1) * dsub] for j in range(m)]).astype(np.float32)
        codes = r.integers(0, K, (n, m)).astype(np.uint16)
        return ia.ProductQuantizer(d, cb), codes

    done = []

    def note(name, idx):
        st = idx.last_stats()
        done.append({"path": name, "exact_path": st["exact_path"], "replayed": st["replayed"], "evals": st["evals"]})

    for d in (40, 768) if part != "recompute" else ():
        n = 3000
        v = rows(n, d, 100 + d)
        q = rows(nq, d, 200 + d)
        qb = q.copy()
        qb[::2] = widen(bf16_bits(q[::2]))  # every other query holds bf16 values: both launches of the pair get work
        b = bf16_bits(v)
        codes8, e8 = ia.quantize_fp8_e4m3(v)
        g24, g100, g140 = csr(n, 24, 1), csr(n, 100, 2), csr(n, 140, 3)

        plain = index(g24, d, lambda i: i.set_embeddings(v))
        plain.search_batch(q, k, 128)
        note(f"plain f32 d={d}", plain)
        plain.search_batch(q, k, 513)
        note(f"ef=513 d={d}", plain)
        plain.select_entry_seeds(16)
        plain.search_batch(q, k, 128)
        note(f"seeded d={d}", plain)

        narrow = index(g24, d, lambda i: i.set_embeddings_bf16(b))
        narrow.search_batch(qb, k, 128)
        note(f"bf16 <= 64 ids d={d}", narrow)
        wide = index(g100, d, lambda i: i.set_embeddings_bf16(b))
        wide.search_batch(qb, k, 128)
        note(f"bf16 65-128 ids d={d}", wide)
        fp8 = index(g24, d, lambda i: i.set_embeddings_fp8(codes8, e8))
        fp8.search_batch(q, k, 128)
        note(f"fp8 d={d}", fp8)
        long_rows = index(g140, d, lambda i: i.set_embeddings(v))
        long_rows.search_batch(q, k, 128)
        note(f"degree 140 d={d}", long_rows)

        m, K = (8, 32) if d == 40 else (96, 64)
        tl = index(g24, d, lambda i: i.set_embeddings(v))
        pq, codes = pq_of(v, m, K, 5)
        tl.set_pq_codes(pq, codes)
        tl.search_two_level_batch(q, k, 64, 0.2)
        note(f"two-level f32 d={d}", tl)
        tlb = index(g24, d, lambda i: i.set_embeddings_bf16(b))
        pqb, codesb = pq_of(widen(b), m, K, 6)
        tlb.set_pq_codes(pqb, codesb)
        tlb.search_two_level_batch(qb, k, 64, 0.2)
        note(f"two-level bf16 d={d}", tlb)
        # the warm launches: plain at two ef, two-level, the group workspaces
        tl.prepare(nq, 128, k, 2)
        tl.search_batch(q, k, 128)
        note(f"prepared d={d}", tl)

        # HnswGraph: the builder's construction searches, then a search that descends
        hv = v[:200]
        for name, h in (("f32", ia.HnswGraph.build(hv, m=8, m0=16, ef_construction=40, level_seed=3)),
                        ("bf16", ia.HnswGraph.build_bf16(bf16_bits(hv), m=8, m0=16, ef_construction=40, level_seed=3))):
            h.search_batch(qb, k, 64)
            done.append({"path": f"hnsw {name} d={d}", "max_level": int(h.max_level)})

    if part == "main":
        print(json.dumps({"calls": done}))
        return
    # the recompute provider: rounds over a bounded row cache (the encoder's d = 64), plain and two-level
    cfg = dict(vocab_size=400, hidden=64, layers=2, heads=4, intermediate=128, max_position=16, type_vocab=2)
    enc = ia.CandleEmbedder(ia.BertConfig(**cfg), bert_ref.random_weights(cfg, seed=45, std=0.2), normalize=True)
    n, L = 1200, 12
    tok = rng.integers(1, 400, (n, L)).astype(np.uint16)
    ids = tok.astype(np.int64)
    emb = np.concatenate([enc.embed(ids[o:o + 256], None, np.ones((min(256, n - o), L), np.float32))
                          for o in range(0, n, 256)])
    g = csr(n, 16, 9)
    for cache in (None, 512):
        q = emb[::17][:nq if cache is None else 6] + np.float32(0.01)  # (a bounded cache serves two queries at a time)
        rec = ia.LeannIndex.from_csr(g, None, dimension=64).upload(0)
        rec.set_recompute_provider(enc, tok, None, cache_rows=cache)
        rec.search_batch(q, k, 48)
        note(f"recompute cache={cache}", rec)
        rec.search_batch(q, k, 600)
        note(f"recompute ef=600 cache={cache}", rec)
        pq, codes = pq_of(emb, 8, 32, 11)
        rec.set_pq_codes(pq, codes)
        rec.search_two_level_batch(q, k, 48, 0.2)
        note(f"recompute two-level cache={cache}", rec)
    print(json.dumps({"calls": done}))


def load(trace_dir):
    files = sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True))
    assert len(files) == 1, files
    with open(files[0]) as f:
        # in the order the host dispatched them (prepare() warms several streams at once: their kernels start in any
        # order, but the one host thread enqueues them in the same one)
        recs = sorted(csv.DictReader(f), key=lambda r: int(r.get("Dispatch_Id") or r["Start_Timestamp"]))
    out = []
    for r in recs:
        name = r["Kernel_Name"]
        if name.startswith("void "):
            name = name[5:]
        # the library's kernels and the runtime's fills behind its memsets; nothing of torch's or rocBLAS's
        if name.startswith(("at::", "Cijk", "rocprim", "hipcub")):
            continue
        out.append([name, "x".join(r[f"Grid_Size_{a}"] for a in "XYZ"), "x".join(r[f"Workgroup_Size_{a}"] for a in "XYZ"),
                    r["LDS_Block_Size"]])
    return out


def compare(a_dir, b_dir, out_path, distinct):
    a, b = load(a_dir), load(b_dir)
    rec = {"what": "rocprofv3 --kernel-trace of tools/launch_trace.py, two builds; the library's dispatches in the order "
                   "the host made them, compared by kernel name, grid, workgroup size and LDS size",
           "dispatches_parent": len(a), "dispatches_branch": len(b)}
    if distinct:
        # the rounds of the recompute provider differ from run to run of ONE build (how many rows a round finds missing,
        # and with it the rounds' number and grids): the instantiations launched are compared, as a set, without grids
        sa, sb = ({(r[0], r[2], r[3]) for r in t} for t in (a, b))
        diff = [{"only_parent": list(x)} for x in sorted(sa - sb)] + [{"only_branch": list(x)} for x in sorted(sb - sa)]
        rec.update(compared="distinct (kernel name, workgroup size, LDS size)", distinct_parent=len(sa),
                   distinct_branch=len(sb), differing_count=len(diff))
    else:
        diff = [{"row": i, "parent": x, "branch": y} for i, (x, y) in enumerate(zip(a, b)) if x != y]
        rec.update(compared="row by row", differing_count=len(diff) + abs(len(a) - len(b)))
    rec["differing_rows"] = diff[:50]
    count = {}
    for r in b:  # dispatches per kernel, template arguments kept (they carry the instantiation), parameters dropped
        name = r[0].replace("(anonymous namespace)::", "").split("(")[0]
        count[name] = count.get(name, 0) + 1
    rec["dispatches_by_kernel_branch"] = dict(sorted(count.items()))
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps({k: v for k, v in rec.items() if k not in ("what", "dispatches_by_kernel_branch", "differing_rows")}))
    for r in diff[:4]:
        print(json.dumps(r))
    return 0 if rec["differing_count"] == 0 else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("main", "recompute", "all"), default="all")
    ap.add_argument("--compare", nargs=2, metavar=("PARENT_DIR", "BRANCH_DIR"))
    ap.add_argument("--distinct", action="store_true", help="compare the sets of instantiations, not the rows")
    ap.add_argument("--out", default="launch_plan_trace_ab.json")
    a = ap.parse_args()
    sys.exit(compare(a.compare[0], a.compare[1], a.out, a.distinct) if a.compare else run(a.part))
