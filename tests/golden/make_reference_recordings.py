"""Records what THE REFERENCE'S OWN CODE computes, for tests/test_reference_recordings.py.

Runs the two probe binaries that oracle/ref_build/ builds around a host compile of the reference's unmodified sources
(oracle/_ref/ref_probe_libm: glibc math; ref_probe_det: sin/cos/pow of the render path bound to oracle/pt_oracle_math.h) over
every case and writes one tests/golden/ref/<case>.npz each, plus bench_frames.json.  DATA only: arrays the reference's
programs wrote while they ran.  Needs the reference's scene files and the probes, so it runs in the build container only;
the tests read the recordings and need neither.

  python tests/golden/make_reference_recordings.py [--out DIR] [--ref DIR] [--only CASE ...]

Per case (keys of the .npz):
  reference            "accepts" | "rejects" (+ message: what the reference's parser threw); a rejected case ends here
  dump_<array>         the reference's Scene after its constructor (ref_probe.cpp lists the arrays), in full for small
                       scenes; for big ones  dumpsha_<array> (SHA-256 of the array's bytes) + dumpshape_<array>
  size                 W, H, SPP of the frames
  frame_libm_per_pixel, frame_libm_per_sample, frame_det_per_sample      float32 [H, W, 3], seed 1984
  rays, hit, hit_ids   1,024 rays (make_golden_vectors.make_rays; for the tie / axis cases the last 256 are axis and
                       coordinate-plane rays with both signs of zero) and the reference's intersect(): hit = distance,
                       position, shading normal; hit_ids = valid, material id, area-light id
  centre_size, centre_dir, centre_hit, centre_ids     the same for the rays through the pixel centres of a 32 x 24 film
"""
import argparse
import hashlib
import json
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
REPO = os.path.dirname(TESTS)
sys.path.insert(0, TESTS)
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

REF_DEFAULT = os.environ.get("PT_REFERENCE_DIR", "/root/reference")      # as __graft_entry__.build_reference_probes
PROBE_DIR = os.path.join(REPO, "oracle", "_ref")
PROBES = {"libm": os.path.join(PROBE_DIR, "ref_probe_libm"), "det": os.path.join(PROBE_DIR, "ref_probe_det")}
OUT_DEFAULT = os.path.join(HERE, "ref")
SEED = 1984
N_RAYS = 1024
CENTRE_SIZE = (32, 24)
FULL_DUMP_BYTES = 96 * 1024          # dumps above this are recorded as hashes (teapot, bunny)

# the 14 shipped scenes: name -> file below <reference>/scenes (make_scene_fixtures.SCENES) and frame size (make_golden_vectors.IMAGES)
from make_golden_vectors import IMAGES as SHIPPED_SIZE  # noqa: E402
from make_scene_fixtures import SCENES as SHIPPED  # noqa: E402

# inputs of our own, relative to tests/data
OWN = {
    "plastic": "ref_cases/plastic.xml",
    "phong": "ref_cases/phong.xml",
    "mirrors": "ref_cases/mirrors.xml",
    "all_materials": "ref_cases/all_materials.xml",
    "emitters": "ref_cases/emitters.xml",
    "inside_sphere": "ref_cases/inside_sphere.xml",
    "meshes": "ref_cases/meshes.xml",
    "ties": "ref_cases/ties.xml",
    "ascii_ply": "ref_cases/ascii_ply.xml",
    "point_light_first": "quirk_point_light_first.xml",
    "mixed": "mixed.xml",
}
OWN_SIZE = (64, 48, 4)
AXIS_RAY_CASES = ("ties", "meshes", "aabb_test", "cbox")
# bench.py's WORKLOADS / BASELINE.json's single-GPU configs
BENCH_FRAMES = {"scene1": (640, 480, 16), "cbox": (640, 480, 64), "bunny": (640, 480, 64)}


def case_names():
    return list(SHIPPED) + list(OWN)


def case_xml(name, ref_dir=REF_DEFAULT):
    if name in SHIPPED:
        return os.path.join(ref_dir, "scenes", SHIPPED[name])
    return os.path.join(TESTS, "data", OWN[name])


def case_size(name):
    return SHIPPED_SIZE[name] if name in SHIPPED else OWN_SIZE


def read_probe_file(path):
    """The probe's container: 'PTRP', then name / type / rank / extents / data per array."""
    b = open(path, "rb").read()
    assert b[:4] == b"PTRP", path
    o, out = 4, {}
    while o < len(b):
        (n,) = struct.unpack_from("<I", b, o)
        name = b[o + 4:o + 4 + n].decode()
        o += 4 + n
        t, rank = struct.unpack_from("<II", b, o)
        ext = struct.unpack_from("<%dI" % rank, b, o + 8)
        o += 8 + 4 * rank
        cnt = int(np.prod(ext, dtype=np.int64))
        out[name] = np.frombuffer(b, dtype="<f4" if t == 0 else "<i4", count=cnt, offset=o).reshape(ext).copy()
        o += 4 * cnt
    return out


class Rejected(Exception):
    pass


def probe(flavour, *args, tmp):
    """Runs one probe command; the last argument of every command is the output file, appended here."""
    out = os.path.join(tmp, "out.bin")
    r = subprocess.run([PROBES[flavour], *[str(a) for a in args], out], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
    if r.returncode == 3:
        raise Rejected(r.stderr.strip().splitlines()[-1].replace("REJECTED: ", "", 1))
    if r.returncode != 0:
        raise RuntimeError(f"{PROBES[flavour]} {args}: exit {r.returncode}: {r.stderr[-400:]}")
    return read_probe_file(out)


def axis_rays(n, seed, lo, hi):
    """Rays along the axes and in the coordinate planes, the zero components of both signs, from points in [lo, hi]."""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((n, 3)).astype(np.float32)
    for k in range(n):
        if k % 2 == 0:
            a = int(rng.integers(0, 3))
            s = d[k, a]
            d[k] = -0.0 if rng.random() < 0.5 else 0.0
            d[k, a] = 1.0 if s > 0 else -1.0
        else:
            d[k, int(rng.integers(0, 3))] = -0.0 if rng.random() < 0.5 else 0.0
            d[k] /= np.linalg.norm(d[k])
    org = (lo + (hi - lo) * rng.random((n, 3))).astype(np.float32)
    # a quarter of the origins on a lattice of "round" coordinates, where box faces and shared edges lie
    org[: n // 4] = np.round(org[: n // 4] * 4) / 4
    rays = np.zeros((n, 8), dtype=np.float32)
    rays[:, :3], rays[:, 3:6], rays[:, 6], rays[:, 7] = org, d, 1e-4, np.finfo(np.float32).max
    return rays


def hashed(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def record_case(name, k, ref_dir, tmp):
    from make_golden_vectors import make_rays
    from pathtracer_cuda_interactive_amd import PT_BVH_SORT_REFERENCE, HostScene

    xml = case_xml(name, ref_dir)
    w, h, spp = case_size(name)
    rec = {}
    try:
        dump = probe("libm", "dump", xml, w, h, tmp=tmp)
    except Rejected as e:
        return {"reference": np.array("rejects"), "message": np.array(str(e))}
    rec["reference"] = np.array("accepts")
    assert all(np.array_equal(v, probe("det", "dump", xml, w, h, tmp=tmp)[kk]) for kk, v in dump.items()), name
    full = sum(v.nbytes for v in dump.values()) <= FULL_DUMP_BYTES
    for key, v in dump.items():
        if full:
            rec["dump_" + key] = v
        else:
            rec["dumpsha_" + key] = np.array(hashed(v))
            rec["dumpshape_" + key] = np.array(v.shape, dtype=np.int64)
    rec["size"] = np.array([w, h, spp], dtype=np.int32)
    for flavour, mode in (("libm", "per_pixel"), ("libm", "per_sample"), ("det", "per_sample")):
        f = probe(flavour, "render", xml, w, h, spp, SEED, mode, tmp=tmp)["frame"]
        # non-finite radiance is outside what is pinned: a case that produces it has to change
        assert np.isfinite(f).all(), f"{name} {flavour}/{mode}: non-finite radiance"
        rec[f"frame_{flavour}_{mode}"] = f

    # rays: the generator of the per-ray KATs, on the scene as OUR pipeline loads it (it only chooses the rays)
    hs = HostScene.load(xml if name in OWN else os.path.join(HERE, "scenes", name + ".pts"))
    d = hs.finalize(PT_BVH_SORT_REFERENCE)
    rays = make_rays(hs, d, N_RAYS, 100 + k)
    if name in AXIS_RAY_CASES:
        box = dump["node_box"][int(dump["root"][0])]
        rays[-256:] = axis_rays(256, 7000 + k, box[:3], box[3:])
    rays_file = os.path.join(tmp, "rays.bin")
    rays.astype("<f4").tofile(rays_file)
    hits = probe("libm", "hits", xml, rays_file, tmp=tmp)
    hits_det = probe("det", "hits", xml, rays_file, tmp=tmp)
    assert all(np.array_equal(hits[kk].view(np.uint32), hits_det[kk].view(np.uint32)) for kk in hits), name
    assert np.array_equal(hits["rays"].view(np.uint32), rays.view(np.uint32))
    assert np.isfinite(hits["hit"]).all(), f"{name}: non-finite hit record"
    rec["rays"], rec["hit"], rec["hit_ids"] = rays, hits["hit"][:, :7], hits["hit_ids"]
    cw, ch = CENTRE_SIZE
    c = probe("libm", "centres", xml, cw, ch, tmp=tmp)
    assert np.isfinite(c["hit"]).all() and np.isfinite(c["rays"][:, :6]).all(), f"{name}: non-finite pixel-centre record"
    rec["centre_size"] = np.array([cw, ch], dtype=np.int32)
    rec["centre_origin"] = c["rays"][0, :3]
    rec["centre_dir"] = c["rays"][:, 3:6]
    rec["centre_hit"] = c["hit"][:, :7]
    rec["centre_ids"] = c["hit_ids"]
    return rec


def record_bench_frames(ref_dir, tmp, names=None):
    out = {}
    for name, (w, h, spp) in BENCH_FRAMES.items():
        if names and name not in names:
            continue
        f = probe("det", "render", case_xml(name, ref_dir), w, h, spp, SEED, "per_sample", tmp=tmp)["frame"]
        assert np.isfinite(f).all(), name
        out[name] = {"width": w, "height": h, "spp": spp, "seed": SEED, "flavour": "det/per_sample", "sha256": hashed(f),
                     "mean": float(f.mean(dtype=np.float64)), "max": float(f.max())}
    return out


def save_npz(path, rec):
    """An .npz np.load reads, written with fixed time stamps: the same arrays give the same file, byte for byte."""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for key, a in rec.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(a, order="C"), version=(1, 0), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def generate(out_dir, ref_dir=REF_DEFAULT, only=None, bench=True):
    os.makedirs(out_dir, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        for k, name in enumerate(case_names()):
            if only and name not in only:
                continue
            rec = record_case(name, k, ref_dir, tmp)
            save_npz(os.path.join(out_dir, name + ".npz"), rec)
            print(name, str(rec["reference"]), os.path.getsize(os.path.join(out_dir, name + ".npz")), "bytes", flush=True)
        if bench and not only:
            with open(os.path.join(out_dir, "bench_frames.json"), "w") as f:
                json.dump(record_bench_frames(ref_dir, tmp), f, indent=1, sort_keys=True)
                f.write("\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT_DEFAULT)
    ap.add_argument("--ref", default=REF_DEFAULT)
    ap.add_argument("--only", nargs="*")
    a = ap.parse_args()
    generate(a.out, a.ref, a.only)
