"""What the row conversions cost on the device, beside a device-to-device copy of the f32 block and beside the
host path they replace.
    python tools/convert_rows_perf.py [--nodes 1000000] [--dim 768] [--runs 5] [--host-rows 131072]
                                      [--out profiles/convert_rows.json]
Dataset M of tools/synth.py, resident on the device.  Every leg is timed with HIP events on the default stream
(the one the calls run on), one warm-up and then the median of `runs`:
  f32 -> fp8 explicit   isl_quantize_fp8_e4m3 with the exponent given: one pass, 5 bytes per element
  f32 -> fp8 auto       ... with ISL_FP8_SCALE_AUTO: the absmax pass in front, 9 bytes per element
  f32 -> bf16           isl_round_bf16: 6 bytes per element
  copy                  hipMemcpyDtoD of the f32 block (torch's copy_): 8 bytes per element
The three calls are the convert kernel over dense buffers plus the 8-byte read-back and the synchronisation every
call ends with.  The index legs time LeannIndex.convert_rows as a whole -- the new table's allocation, the convert
pass, the norms of the new rows and the release of the old table -- over a ring graph of the same rows:
  index f32 -> fp8, fp8 -> f32, f32 -> bf16, bf16 -> f32
Host path: ia.quantize_fp8_e4m3 (numpy, float64) over the first `host-rows` rows plus set_embeddings_fp8 of those
codes, wall clock, and that time scaled to all rows (the quantiser is linear in the element count)."""
import argparse, json, os, statistics, sys, time
sys.path[:0] = [os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]
import numpy as np, torch
import islands_amd as ia
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import synth

ap = argparse.ArgumentParser()
ap.add_argument("--nodes", type=int, default=1_000_000)
ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--host-rows", type=int, default=131072)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                               "convert_rows.json"))
args = ap.parse_args()
N, d = args.nodes, args.dim
dev = torch.device("cuda:0")
x = synth.make_manifold(N, d, 42, device=dev)
codes = torch.zeros((N, d), dtype=torch.uint8, device=dev)
half = torch.zeros((N, d), dtype=torch.int16, device=dev)
other = torch.zeros_like(x)
torch.cuda.synchronize()
e_auto = ia.quantize_fp8_e4m3_device(device_ptr=x.data_ptr(), out_ptr=codes.data_ptr(), n=N, d=d)


def timed(call):
    """median HIP-event milliseconds of `runs` calls after one warm-up, and every run"""
    ms = []
    for i in range(args.runs + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        call()
        b.record()
        b.synchronize()
        if i:
            ms.append(a.elapsed_time(b))
    return statistics.median(ms), ms


def leg(name, call, bytes_per_elem):
    med, runs = timed(call)
    return {"leg": name, "bytes_per_element": bytes_per_elem, "ms_median": round(med, 4), "ms_runs": [round(v, 4) for v in runs],
            "bytes_per_s": round(N * d * bytes_per_elem / (med / 1e3))}


legs = [
    leg("f32 -> fp8 explicit", lambda: ia.quantize_fp8_e4m3_device(scale_exp=e_auto, device_ptr=x.data_ptr(),
                                                                  out_ptr=codes.data_ptr(), n=N, d=d), 5),
    leg("f32 -> fp8 auto", lambda: ia.quantize_fp8_e4m3_device(device_ptr=x.data_ptr(), out_ptr=codes.data_ptr(), n=N, d=d), 9),
    leg("f32 -> bf16", lambda: ia.round_bf16_device(device_ptr=x.data_ptr(), out_ptr=half.data_ptr(), n=N, d=d), 6),
    leg("copy f32 block (hipMemcpyDtoD)", lambda: other.copy_(x), 8),
]
copy_ms = legs[-1]["ms_median"]
for l in legs:
    l["times_the_copy"] = round(l["ms_median"] / copy_ms, 3)
del other, half

# the index legs: a ring graph, the rows attached by device pointer
off = np.arange(N + 1, dtype=np.uint64)
g = ia.CsrGraph(node_offsets=off, neighbors=((np.arange(N, dtype=np.uint64) + 1) % N), levels=np.zeros(N, np.uint64),
                entry_point=0, num_nodes=N, degree_counts=np.ones(N, np.uint64))
idx = ia.LeannIndex.from_csr(g, ia.LeannConfig(m=8, m0=16, ef_construction=40), dimension=d).upload(0)
idx.set_embeddings(None, device_ptr=x.data_ptr(), n=N, d=d)


def there_and_back(target, scale_exp):
    """(ms of f32 -> target, ms of target -> f32), each the median of `runs` after one warm-up round trip"""
    to, back = [], []
    for i in range(args.runs + 1):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        torch.cuda.synchronize()
        ev[0].record()
        idx.convert_rows(target, scale_exp=scale_exp)
        ev[1].record()
        idx.convert_rows("f32")
        ev[2].record()
        ev[2].synchronize()
        if i:
            to.append(ev[0].elapsed_time(ev[1]))
            back.append(ev[1].elapsed_time(ev[2]))
        # (fp8: the images went back, so the next round narrows the images -- the same work)
    return to, back


index_legs = []
for target, e, b_to, b_back in (("fp8", e_auto, 5, 5), ("bf16", None, 6, 6)):
    to, back = there_and_back(target, e)
    for name, runs, bpe in ((f"index f32 -> {target}", to, b_to), (f"index {target} -> f32", back, b_back)):
        med = statistics.median(runs)
        index_legs.append({"leg": name, "convert_pass_bytes_per_element": bpe, "ms_median": round(med, 4),
                           "ms_runs": [round(v, 4) for v in runs], "times_the_copy": round(med / copy_ms, 3),
                           "includes": "allocation of the new table, convert pass, norms of the new rows, release of the old table"})

# the host path this replaces, on a slice
hn = min(args.host_rows, N)
xh = x[:hn].cpu().numpy()
small = ia.LeannIndex.from_csr(ia.CsrGraph(node_offsets=off[:hn + 1], neighbors=((np.arange(hn, dtype=np.uint64) + 1) % hn),
                                           levels=np.zeros(hn, np.uint64), entry_point=0, num_nodes=hn,
                                           degree_counts=np.ones(hn, np.uint64)),
                               ia.LeannConfig(m=8, m0=16, ef_construction=40), dimension=d).upload(0)
t0 = time.time()
hc, he = ia.quantize_fp8_e4m3(xh)
t1 = time.time()
small.set_embeddings_fp8(hc, he)
t2 = time.time()
same = bool((codes[:hn].cpu().numpy() == ia.quantize_fp8_e4m3(xh, scale_exp=e_auto)[0]).all())
result = {"what": "convert_rows_perf", "dataset": "M", "nodes": N, "dim": d, "runs": args.runs, "fp8_scale_exp": e_auto,
          "timer": "HIP events on the default stream around each call; median after one warm-up",
          "stand_alone": legs, "index": index_legs,
          "host_path": {"rows_measured": hn, "quantize_s": round(t1 - t0, 3), "set_embeddings_fp8_s": round(t2 - t1, 3),
                        "seconds_scaled_to_all_rows": round((t2 - t0) * N / hn, 2), "timer": "wall clock"},
          "device_codes_equal_host_codes_on_the_slice": same}
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print(json.dumps(result), flush=True)
