"""Model-file timing (gsr_model, csrc/modelio.hip) at 1M Gaussians / SH 3 / SG 0 and 5M / SH 3 / SG 7.

  pack / unpack   one call on tensors already on the device (device events around `reps` calls, median over
                  `rounds` windows with the min-max spread), the achieved GB/s on 2 P A 4 bytes (every word read
                  once and written once) and its share of the 8 TB/s HBM peak and of the 6.3 TB/s a streaming
                  kernel achieves.  The unpack call reads its two column tables back before it launches, so its
                  window holds that wait as well; `unpack_call_floor` is the same call at P = 1, the wait alone.
  torch_chain     the same rows by transpose -> flatten -> contiguous -> cat on the same GPU, with the peak of
                  torch.cuda.max_memory_allocated above the inputs (the rows themselves and the temporaries);
  host_reference  at 100k Gaussians, the reference's save_ply body restated: .cpu() per tensor, np.concatenate,
                  list(map(tuple, ...)) into the structured array (host clock) — the only baseline there is;
  save_ply / load_ply   the whole call (host clock, synchronised), next to the time the file system alone takes
                  to write and read that many bytes from a host buffer.  The file system is where a save or a load
                  spends its time; the kernel time is not the user's time.
Also records that the packed rows equal the torch chain's bit for bit at each size.
Writes profiles/modelio_bench.json (or --out) and prints it as one JSON line.

    python tools/bench_modelio.py [--rounds 5] [--reps 10] [--dir /tmp] [--out profiles/modelio_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "geometry-grounded-gaussian-splatting_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import gsr_model  # noqa: E402
import gsr_scene as S  # noqa: E402
from diff_gaussian_rasterization import _abi  # noqa: E402

PEAK_TBPS, STREAM_TBPS = 8.0, 6.3
SIZES = [("1M_sh3_sg0", 1_000_000, 3, 0), ("5M_sh3_sg7", 5_000_000, 3, 7)]


def spread(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def device_windows(fn, rounds, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        t.append(e0.elapsed_time(e1) / reps)
    return spread(t)


def host_windows(fn, rounds, warmup=1):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return spread(t)


def rate(res, nbytes):
    gbps = nbytes / (res["median_ms"] * 1e-3) / 1e9
    return dict(res, gbps=round(gbps, 1), share_of_peak=round(gbps / (PEAK_TBPS * 1e3), 4),
                share_of_stream=round(gbps / (STREAM_TBPS * 1e3), 4))


def random_model(P, sh, sg, dev):
    g = torch.Generator(device=dev).manual_seed(P + sh + sg)
    M = (sh + 1) ** 2
    shapes = ((P, 3), (P, 1, 3), (P, M - 1, 3), (P, 3), (P, 4), (P, 1), (P, sg, 3), (P, sg), (P, sg, 3), (P, 1))
    return S.RawGaussians(*[torch.randn(s, generator=g, device=dev) for s in shapes])


def torch_chain(raw):
    return torch.cat((raw.xyz, torch.zeros_like(raw.xyz), raw.features_dc.transpose(1, 2).flatten(1).contiguous(),
                      raw.features_rest.transpose(1, 2).flatten(1).contiguous(), raw.opacity, raw.scaling,
                      raw.rotation, raw.sg_axis.flatten(1).contiguous(), raw.sg_sharpness,
                      raw.sg_color.flatten(1).contiguous(), raw.filter_3D), dim=1)


def host_reference(raw, names):
    """save_ply's body up to the structured array (gaussian_model.py:475-491)."""
    xyz = raw.xyz.detach().cpu().numpy()
    normals = np.zeros_like(xyz)
    f_dc = raw.features_dc.detach().transpose(1, 2).flatten(start_dim=1).contiguous().cpu().numpy()
    f_rest = raw.features_rest.detach().transpose(1, 2).flatten(start_dim=1).contiguous().cpu().numpy()
    opacities = raw.opacity.detach().cpu().numpy()
    scale = raw.scaling.detach().cpu().numpy()
    rotation = raw.rotation.detach().cpu().numpy()
    sg_axis = raw.sg_axis.detach().flatten(start_dim=1).contiguous().cpu().numpy()
    sg_sharpness = raw.sg_sharpness.detach().cpu().numpy()
    sg_color = raw.sg_color.detach().flatten(start_dim=1).contiguous().cpu().numpy()
    filter_3D = raw.filter_3D.detach().cpu().numpy()
    elements = np.empty(xyz.shape[0], dtype=[(n, "f4") for n in names])
    attributes = np.concatenate((xyz, normals, f_dc, f_rest, opacities, scale, rotation, sg_axis, sg_sharpness,
                                 sg_color, filter_3D), axis=1)
    elements[:] = list(map(tuple, attributes))
    return elements


def bench_size(P, sh, sg, dev, args, folder):
    L = _abi.load()
    raw = random_model(P, sh, sg, dev)
    tensors, _, M, G = gsr_model._tensors(raw)
    A = gsr_model.row_floats(M, G)
    nbytes = 2 * P * A * 4
    rows = torch.empty(P * A, dtype=torch.float32, device=dev)
    res = {"P": P, "sh_degree": sh, "sg_degree": sg, "row_floats": A, "bytes_moved": nbytes,
           "block_rows": L.gsr_model_block_rows(A)}
    res["pack"] = rate(device_windows(lambda: gsr_model.pack_rows(tensors, M, G, out=rows), args.rounds, args.reps),
                       nbytes)
    # unpack of the canonical rows into fresh tensors
    h = gsr_model.PlyHeader(P, [(n, "float", 4 * k) for k, n in enumerate(gsr_model.attribute_names(M, G))], 4 * A,
                            0, sh, G, True)
    off, code = (torch.from_numpy(a).to(dev) for a in h.column_tables())
    outs = [torch.empty_like(t) for t in tensors]
    st = _abi.stream(dev)

    def unpack(n=P):
        _abi.check(L.gsr_model_unpack_rows(n, M, G, 4 * A, rows.data_ptr(), off.data_ptr(), code.data_ptr(),
                                           *gsr_model._ptrs(outs, 0, n), st))

    res["unpack"] = rate(device_windows(unpack, args.rounds, args.reps), nbytes)
    res["unpack_call_floor"] = device_windows(lambda: unpack(1), args.rounds, args.reps)
    res["unpack_bits_equal"] = all(torch.equal(a.view(torch.int32), b.view(torch.int32))
                                   for a, b in zip(outs, tensors))
    del outs
    # the torch chain
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    want = torch_chain(raw)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - base
    res["pack_bits_equal_torch_chain"] = bool(torch.equal(want.view(torch.int32), rows.view(P, A).view(torch.int32)))
    del want
    res["torch_chain"] = rate(device_windows(lambda: torch_chain(raw), args.rounds, args.reps), nbytes)
    res["torch_chain"]["peak_extra_bytes"] = int(peak)
    res["torch_chain"]["peak_extra_bytes_beyond_rows"] = int(peak - P * A * 4)
    res["torch_chain_over_pack"] = round(res["torch_chain"]["median_ms"] / res["pack"]["median_ms"], 3)
    del rows
    # whole calls, and the file system alone on the same bytes
    path = os.path.join(folder, f"m{P}.ply")
    res["save_ply"] = host_windows(lambda: gsr_model.save_ply(raw, path), args.file_rounds)
    res["load_ply"] = host_windows(lambda: gsr_model.load_ply(path, device=dev), args.file_rounds)
    size = os.path.getsize(path)
    buf = np.zeros(gsr_model.CHUNK_BYTES, dtype=np.uint8)
    scratch = os.path.join(folder, "fs.bin")

    def fs_write():
        with open(scratch, "wb") as f:
            for k in range(0, size, buf.size):
                f.write(buf[:min(buf.size, size - k)].data)

    def fs_read():
        with open(scratch, "rb") as f:
            for k in range(0, size, buf.size):
                f.readinto(buf[:min(buf.size, size - k)])

    res["file_bytes"] = size
    res["fs_write_alone"] = host_windows(fs_write, args.file_rounds)
    res["fs_read_alone"] = host_windows(fs_read, args.file_rounds)
    res["fs_share_of_save"] = round(res["fs_write_alone"]["median_ms"] / res["save_ply"]["median_ms"], 3)
    res["fs_share_of_load"] = round(res["fs_read_alone"]["median_ms"] / res["load_ply"]["median_ms"], 3)
    res["pack_share_of_save"] = round(res["pack"]["median_ms"] / res["save_ply"]["median_ms"], 5)
    os.remove(path)
    os.remove(scratch)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--file-rounds", type=int, default=3)
    ap.add_argument("--dir", default=None, help="where the files are written (default: a temporary directory)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "modelio_bench.json"))
    ap.add_argument("--sizes", default=",".join(s[0] for s in SIZES))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_modelio needs a HIP device"
    dev = torch.device("cuda", 0)
    res = {"device": torch.cuda.get_device_name(0), "peak_tbps": PEAK_TBPS, "stream_tbps": STREAM_TBPS}
    with tempfile.TemporaryDirectory(dir=args.dir) as folder:
        for name, P, sh, sg in SIZES:
            if name in args.sizes.split(","):
                res[name] = bench_size(P, sh, sg, dev, args, folder)
                torch.cuda.empty_cache()
        # the reference's host path at 100k
        raw = random_model(100_000, 3, 0, dev)
        names = gsr_model.attribute_names(16, 0)
        tensors, _, M, G = gsr_model._tensors(raw)
        ref = host_windows(lambda: host_reference(raw, names), 3)
        pack = device_windows(lambda: gsr_model.pack_rows(tensors, M, G), args.rounds, args.reps)

        def pack_to_host():
            return gsr_model.pack_rows(tensors, M, G).cpu()

        got = pack_to_host().numpy()
        el = host_reference(raw, names)
        same = all(np.array_equal(el[n].view(np.uint32), got[:, k].view(np.uint32)) for k, n in enumerate(names))
        res["100k_sh3_sg0"] = {"host_reference": ref, "pack": pack, "pack_and_copy_to_host": host_windows(pack_to_host, 5),
                               "rows_equal_host_reference": bool(same)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fp:
        json.dump(res, fp, indent=1)
        fp.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
