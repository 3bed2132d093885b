"""A numpy restatement of the reference's model files (scene/gaussian_model.py:450-493, 541-611): both
directions of point_cloud.ply without plyfile, and the test models of tests/test_modelio.py and
tests/test_gpu_modelio.py.

save_bytes(raw): the header plyfile writes for the reference's all-f4 structured array, then the rows, built as
save_ply builds them: transpose(1, 2).flatten(1) of the two SH tensors, plain flattens of the rest, one
concatenate along axis 1.
load(data): the header parsed into a numpy structured dtype and every column read by name into a float64
array that is then cast to float32, as load_ply does through np.zeros(...) and torch.tensor(..., dtype=float).

`raw` is a dict of the ten stored tensors as float32 arrays (FIELDS).  Comparisons are on the uint32 view.
"""
from __future__ import annotations

import numpy as np

FIELDS = ("xyz", "features_dc", "features_rest", "opacity", "scaling", "rotation", "sg_axis", "sg_sharpness",
          "sg_color", "filter_3D")
# bit patterns that any arithmetic on the way would damage: quiet NaNs with payloads (both signs), -0, the
# infinities, the smallest and the largest denormal.  (Signalling NaNs are left out: the reference's own path
# through float64 quiets them, so `load` could not return them.)
SPECIALS = np.array([0x7FC12345, 0xFFC00001, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF, 0x7FFFFFFF],
                    dtype=np.uint32)
_NP = {"char": "i1", "uchar": "u1", "short": "<i2", "ushort": "<u2", "int": "<i4", "uint": "<u4", "float": "<f4",
       "double": "<f8", "int8": "i1", "uint8": "u1", "int16": "<i2", "uint16": "<u2", "int32": "<i4", "uint32": "<u4",
       "float32": "<f4", "float64": "<f8"}


def shapes(P, M, G):
    return {"xyz": (P, 3), "features_dc": (P, 1, 3), "features_rest": (P, M - 1, 3), "opacity": (P, 1),
            "scaling": (P, 3), "rotation": (P, 4), "sg_axis": (P, G, 3), "sg_sharpness": (P, G),
            "sg_color": (P, G, 3), "filter_3D": (P, 1)}


def make_raw(P, sh_degree, sg_degree, seed=0, special_rows=()):
    """A model of P Gaussians with normal random values; every tensor's rows `special_rows` (those inside
    [0, P)) are overwritten with SPECIALS, starting at a different one per tensor and row."""
    rng = np.random.default_rng(seed)
    M = (sh_degree + 1) ** 2
    raw = {k: rng.standard_normal(s).astype(np.float32) for k, s in shapes(P, M, sg_degree).items()}
    for n, k in enumerate(FIELDS):
        if raw[k].size == 0:
            continue
        flat = raw[k].reshape(P, -1).view(np.uint32)
        for r in special_rows:
            if 0 <= r < P:
                flat[r] = SPECIALS[(np.arange(flat.shape[1]) + n + r) % len(SPECIALS)]
    return raw


def degrees(raw):
    return raw["features_rest"].shape[1] + 1, raw["sg_sharpness"].shape[1]


def names(M, G, exclude_filter=False):
    """construct_list_of_attributes (gaussian_model.py:450-470)."""
    l = ["x", "y", "z", "nx", "ny", "nz"]
    for i in range(1 * 3):
        l.append("f_dc_{}".format(i))
    for i in range((M - 1) * 3):
        l.append("f_rest_{}".format(i))
    l.append("opacity")
    for i in range(3):
        l.append("scale_{}".format(i))
    for i in range(4):
        l.append("rot_{}".format(i))
    for i in range(G * 3):
        l.append("sg_axis_{}".format(i))
    for i in range(G):
        l.append("sg_sharpness_{}".format(i))
    for i in range(G * 3):
        l.append("sg_color_{}".format(i))
    if not exclude_filter:
        l.append("filter_3D")
    return l


def rows(raw):
    """The `attributes` array of save_ply (gaussian_model.py:475-490): [P, A] float32."""
    xyz = raw["xyz"]
    P = xyz.shape[0]
    normals = np.zeros_like(xyz)
    flatten = lambda a: a.reshape(P, a.shape[1] * a.shape[2])  # noqa: E731  (flatten(start_dim=1), also at P = 0)
    f_dc = flatten(np.ascontiguousarray(raw["features_dc"].transpose(0, 2, 1)))
    f_rest = flatten(np.ascontiguousarray(raw["features_rest"].transpose(0, 2, 1)))
    sg_axis = flatten(raw["sg_axis"])
    sg_color = flatten(raw["sg_color"])
    return np.concatenate((xyz, normals, f_dc, f_rest, raw["opacity"], raw["scaling"], raw["rotation"], sg_axis,
                           raw["sg_sharpness"], sg_color, raw["filter_3D"]), axis=1)


def header(count, properties):
    """plyfile's header for one vertex element of `properties` [(name, PLY type)]."""
    lines = ["ply", "format binary_little_endian 1.0", "element vertex %d" % count]
    lines += ["property %s %s" % (t, n) for n, t in properties]
    return ("\n".join(lines) + "\nend_header\n").encode("ascii")


def save_bytes(raw):
    M, G = degrees(raw)
    att = rows(raw)
    return header(att.shape[0], [(n, "float") for n in names(M, G)]) + att.astype("<f4").tobytes()


def parse_header(data):
    """(count, [(name, PLY type)], payload offset) of a binary little-endian PLY with one vertex element first."""
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0", lines[:2]
    assert lines[2].startswith("element vertex ")
    count = int(lines[2].split()[2])
    props = []
    for ln in lines[3:]:
        if not ln.startswith("property "):
            break
        _, t, n = ln.split()
        props.append((n, t))
    return count, props, end


def read_structured(data):
    count, props, end = parse_header(data)
    dtype = np.dtype([(n, _NP[t]) for n, t in props])
    return np.frombuffer(data, dtype=dtype, count=count, offset=end), [n for n, _ in props]


def load(data, allow_missing_filter=False):
    """load_ply (gaussian_model.py:541-608) on the bytes of a file: the ten tensors as float32 arrays."""
    el, prop_names = read_structured(data)
    P = el.shape[0]

    def family(prefix):
        found = [n for n in prop_names if n.startswith(prefix)]
        return sorted(found, key=lambda x: int(x.split("_")[-1]))

    def columns(found):
        out = np.zeros((P, len(found)))  # float64, as the reference's np.zeros
        for idx, n in enumerate(found):
            out[:, idx] = np.asarray(el[n])
        return out

    with np.errstate(over="ignore", under="ignore"):
        f32 = lambda a: a.astype(np.float32)  # noqa: E731  (torch.tensor(a, dtype=torch.float): nearest even)
        xyz = f32(columns(["x", "y", "z"]))
        opacity = f32(columns(["opacity"]))
        if "filter_3D" in prop_names or not allow_missing_filter:
            filter_3D = f32(columns(["filter_3D"]))
        else:
            filter_3D = np.zeros((P, 1), np.float32)
        features_dc = f32(columns(["f_dc_0", "f_dc_1", "f_dc_2"])).reshape(P, 3, 1).transpose(0, 2, 1)
        rest = family("f_rest_")
        K = len(rest) // 3
        assert len(rest) == 3 * K
        features_rest = f32(columns(rest)).reshape(P, 3, K).transpose(0, 2, 1)
        axis, sharp, color = family("sg_axis_"), family("sg_sharpness_"), family("sg_color_")
        G = len(sharp)
        assert len(axis) == 3 * G and len(color) == 3 * G
        out = {"xyz": xyz, "features_dc": features_dc, "features_rest": features_rest, "opacity": opacity,
               "scaling": f32(columns(family("scale_"))), "rotation": f32(columns(family("rot_"))),
               "sg_axis": f32(columns(axis)).reshape(P, G, 3), "sg_sharpness": f32(columns(sharp)),
               "sg_color": f32(columns(color)).reshape(P, G, 3), "filter_3D": filter_3D}
    return {k: np.ascontiguousarray(v) for k, v in out.items()}


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def awkward_doubles(x32, seed=0):
    """float64 values near the float32 values `x32` that no float32 holds: exact ties between two neighbours
    (nearest-even decides), values just off a float32, and a few at the ends of the range (overflow to inf,
    a float32 denormal, underflow to 0)."""
    x32 = np.where(np.isfinite(x32), x32, np.float32(0.5)).astype(np.float32)  # (NaN payloads through float64
    x = x32.astype(np.float64)                                                  # are not part of any contract)
    flat = x.reshape(-1)
    idx = np.arange(flat.size)
    up = np.nextafter(x32.reshape(-1), np.float32(np.inf)).astype(np.float64)
    flat[:] = np.where(idx % 3 == 0, (flat + up) * 0.5, np.where(idx % 3 == 1, flat * (1 + 2.0 ** -30),
                                                                 flat * (1 - 2.0 ** -27)))
    ends = [1e300, -1e300, 1e-42, -3e-45, 1e-60, 3.4028235677973366e38, 0.1]
    flat[:len(ends)] = ends[:flat.size]
    return x


def build_file(raw, reverse=False, uchar_after_z=False, double_prefixes=(), drop_sg=False, drop_filter=False,
               seed=0):
    """A model file in another layout than save_ply's: the property order reversed, three uchar properties
    after z (an odd stride), the columns named by `double_prefixes` stored as double with awkward_doubles'
    values, the SG or filter_3D properties left out.  Returns the file's bytes."""
    M, G = degrees(raw)
    att = rows(raw)
    P = att.shape[0]
    rng = np.random.default_rng(seed + 1)
    props, values = [], {}
    for c, n in enumerate(names(M, G)):
        if drop_sg and n.startswith("sg_"):
            continue
        if drop_filter and n == "filter_3D":
            continue
        if any(n.startswith(p) for p in double_prefixes):
            props.append((n, "double"))
            values[n] = awkward_doubles(att[:, c], seed + c)
        else:
            props.append((n, "float"))
            values[n] = att[:, c]
        if uchar_after_z and n == "z":
            for colour in ("red", "green", "blue"):
                props.append((colour, "uchar"))
                values[colour] = rng.integers(0, 256, P, dtype=np.uint8)
    if reverse:
        props = props[::-1]
    el = np.zeros(P, dtype=np.dtype([(n, _NP[t]) for n, t in props]))
    for n, _ in props:
        el[n] = values[n]
    return header(P, props) + el.tobytes()
