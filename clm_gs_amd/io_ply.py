"""3DGS .ply exchange format without plyfile (scope row f2; reference:
strategies/base_gaussian_model.py:165-248 save_ply / load_raw_ply).

Binary little-endian, one float32 property per attribute, in the reference's order:
x y z nx ny nz f_dc_0..2 f_rest_0..44 opacity scale_0..2 rot_0..3.  f_rest is CHANNEL-major
(index = c * 15 + (k - 1), from .view(-1,15,3).transpose(1,2).flatten(1) at :214-223) while the
in-memory SH row is coefficient-major (index = k * 3 + c).
"""
import numpy as np
import torch


def attribute_names():
    names = ["x", "y", "z", "nx", "ny", "nz"]
    names += [f"f_dc_{i}" for i in range(3)]
    names += [f"f_rest_{i}" for i in range(45)]
    names += ["opacity"] + [f"scale_{i}" for i in range(3)] + [f"rot_{i}" for i in range(4)]
    return names


def save_ply(path, xyz, shs48, opacity, scaling, rotation):
    """All inputs are the STORED parameters (logit opacity, log scale, raw quaternion)."""
    xyz, shs48, opacity, scaling, rotation = (
        t.detach().float().cpu().numpy() for t in (xyz, shs48, opacity, scaling, rotation))
    n = xyz.shape[0]
    sh = shs48.reshape(n, 16, 3)
    f_dc = sh[:, 0, :]                                     # [n,3]  (c)
    f_rest = sh[:, 1:, :].transpose(0, 2, 1).reshape(n, 45)  # [n, c*15 + (k-1)]
    cols = np.concatenate([xyz, np.zeros_like(xyz), f_dc, f_rest, opacity.reshape(n, 1),
                           scaling.reshape(n, 3), rotation.reshape(n, 4)], axis=1).astype("<f4")
    names = attribute_names()
    assert cols.shape[1] == len(names) == 62
    header = "ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % n
    header += "".join("property float %s\n" % a for a in names) + "end_header\n"
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(np.ascontiguousarray(cols).tobytes())


def load_ply(path):
    """-> dict(xyz[n,3], shs48[n,48], opacity[n,1], scaling[n,3], rotation[n,4]) float32 tensors.
    Properties are located by NAME (as load_raw_ply does), so extra / reordered columns are fine."""
    with open(path, "rb") as f:
        assert f.readline().strip() == b"ply"
        fmt = f.readline().decode().split()
        assert fmt[1] == "binary_little_endian", fmt
        props, n = [], None
        while True:
            line = f.readline().decode().strip()
            if line == "end_header":
                break
            tok = line.split()
            if tok[0] == "element":
                assert tok[1] == "vertex"
                n = int(tok[2])
            elif tok[0] == "property":
                assert tok[1] in ("float", "float32"), line
                props.append(tok[2])
        data = np.frombuffer(f.read(n * len(props) * 4), dtype="<f4").reshape(n, len(props))
    col = {p: i for i, p in enumerate(props)}
    get = lambda names: np.stack([data[:, col[a]] for a in names], axis=1)
    n_rest = len([p for p in props if p.startswith("f_rest_")])
    assert n_rest == 45, "SH degree 3 expected (3*(3+1)^2 - 3 = 45 f_rest properties)"
    sh = np.zeros((n, 16, 3), np.float32)
    sh[:, 0, :] = get(["f_dc_0", "f_dc_1", "f_dc_2"])
    sh[:, 1:, :] = get([f"f_rest_{i}" for i in range(45)]).reshape(n, 3, 15).transpose(0, 2, 1)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return dict(xyz=t(get(["x", "y", "z"])), shs48=t(sh.reshape(n, 48)), opacity=t(get(["opacity"])),
                scaling=t(get(["scale_0", "scale_1", "scale_2"])),
                rotation=t(get(["rot_0", "rot_1", "rot_2", "rot_3"])))


def load_model(path):
    """A finished model by its extension: .ply -> load_ply, .npz (a compressed model, clm_gs_amd/compress.py) ->
    compress.load_compressed; both return load_ply's dict."""
    p = str(path).lower()
    if p.endswith(".ply"):
        return load_ply(path)
    if p.endswith(".npz"):
        from .compress import load_compressed
        return load_compressed(path)
    raise ValueError(f"{path}: a model file is a .ply or a compressed .npz")


_MESH_VERTEX = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
_MESH_VERTEX_NORMALS = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
                                 ("red", "u1"), ("green", "u1"), ("blue", "u1")])
_MESH_FACE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])


def _host(a, dtype):
    return np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=dtype)


def save_mesh_ply(path, verts, colours, faces, normals=None):
    """A triangle mesh (clm_gs_amd/tsdf.py) as a binary little-endian .ply: vertex properties x y z (float) and red green
    blue (uchar), faces as `property list uchar int vertex_indices`.  verts [V,3], colours [V,3] in 0..255, faces [F,3]
    (tensors or arrays); V = F = 0 is a valid, empty mesh.  With normals (float32 [V,3]) the vertex element is x y z nx ny
    nz red green blue, the property order MeshLab and open3d write; without them the file is what it always was."""
    verts, colours, faces = _host(verts, np.float32), _host(colours, np.uint8), _host(faces, np.int32)
    verts, colours, faces = verts.reshape(-1, 3), colours.reshape(-1, 3), faces.reshape(-1, 3)
    if len(colours) != len(verts):
        raise ValueError(f"save_mesh_ply: {len(verts)} vertices and {len(colours)} colours")
    if len(faces) and (int(faces.min()) < 0 or int(faces.max()) >= len(verts)):
        raise ValueError(f"save_mesh_ply: a face index lies outside [0, {len(verts)})")
    if normals is not None:
        normals = _host(normals, np.float32)
        if normals.shape != verts.shape:
            raise ValueError(f"save_mesh_ply: normals must be float32 [{len(verts)},3], got {tuple(normals.shape)}")
    v = np.empty(len(verts), dtype=_MESH_VERTEX if normals is None else _MESH_VERTEX_NORMALS)
    for k, name in enumerate(("x", "y", "z")):
        v[name] = verts[:, k]
    for k, name in enumerate(("red", "green", "blue")):
        v[name] = colours[:, k]
    for k, name in enumerate(("nx", "ny", "nz") if normals is not None else ()):
        v[name] = normals[:, k]
    f = np.empty(len(faces), dtype=_MESH_FACE)
    f["n"], f["v"] = 3, faces
    header = "ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % len(v)
    header += "property float x\nproperty float y\nproperty float z\n"
    if normals is not None:
        header += "property float nx\nproperty float ny\nproperty float nz\n"
    header += "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    header += "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % len(f)
    with open(path, "wb") as out:
        out.write(header.encode("ascii"))
        out.write(v.tobytes())
        out.write(f.tobytes())


_MESH_PROPS = ["float x", "float y", "float z", "uchar red", "uchar green", "uchar blue"]
_MESH_PROPS_NORMALS = _MESH_PROPS[:3] + ["float nx", "float ny", "float nz"] + _MESH_PROPS[3:]


def load_mesh_ply(path, with_normals=False):
    """Inverse of save_mesh_ply -> (verts float32 [V,3], colours uint8 [V,3], faces int32 [F,3]) numpy arrays; with
    with_normals a fourth item, the normals float32 [V,3] or None when the file has none.  Reads the two layouts
    save_mesh_ply writes (triangles only); anything else is refused by name."""
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply" or f.readline().decode().split()[1:2] != ["binary_little_endian"]:
            raise ValueError(f"{path}: a binary little-endian .ply expected")
        counts, props, element = {}, {}, None
        while True:
            tok = f.readline().decode().split()
            if tok[:1] == ["end_header"]:
                break
            if tok[:1] == ["element"]:
                element = tok[1]
                counts[element], props[element] = int(tok[2]), []
            elif tok[:1] == ["property"]:
                props[element].append(" ".join(tok[1:]))
        if props.get("vertex") not in (_MESH_PROPS, _MESH_PROPS_NORMALS) or \
                props.get("face") != ["list uchar int vertex_indices"]:
            raise ValueError(f"{path}: not a mesh written by save_mesh_ply (properties {props})")
        vertex = _MESH_VERTEX if props["vertex"] == _MESH_PROPS else _MESH_VERTEX_NORMALS
        v = np.frombuffer(f.read(counts["vertex"] * vertex.itemsize), dtype=vertex)
        fc = np.frombuffer(f.read(counts["face"] * _MESH_FACE.itemsize), dtype=_MESH_FACE)
    if len(v) != counts["vertex"] or len(fc) != counts["face"] or (len(fc) and not (fc["n"] == 3).all()):
        raise ValueError(f"{path}: truncated, or a face that is no triangle")
    verts = np.stack([v["x"], v["y"], v["z"]], axis=1).astype(np.float32).reshape(-1, 3)
    colours = np.stack([v["red"], v["green"], v["blue"]], axis=1).astype(np.uint8).reshape(-1, 3)
    faces = np.ascontiguousarray(fc["v"], dtype=np.int32).reshape(-1, 3)
    if not with_normals:
        return verts, colours, faces
    normals = None
    if vertex is _MESH_VERTEX_NORMALS:
        normals = np.stack([v["nx"], v["ny"], v["nz"]], axis=1).astype(np.float32).reshape(-1, 3)
    return verts, colours, faces, normals


_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2",
              "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4",
              "double": "f8", "float64": "f8"}


def _reference_header(f, path):
    """-> (format, [(element, count, [property tokens after the word `property`])]) of a .ply, in file order."""
    if f.readline().strip() != b"ply":
        raise ValueError(f"{path}: not a .ply file")
    fmt, elements = None, []
    while True:
        line = f.readline()
        if not line:
            raise ValueError(f"{path}: truncated: the header has no end_header")
        tok = line.decode("ascii", "replace").split()
        if tok[:1] == ["end_header"]:
            break
        if tok[:1] == ["format"]:
            fmt = tok[1] if len(tok) > 1 else None
        elif tok[:1] == ["element"] and len(tok) == 3:
            elements.append((tok[1], int(tok[2]), []))
        elif tok[:1] == ["property"] and elements:
            elements[-1][2].append(tok[1:])
    if fmt == "binary_big_endian":
        raise ValueError(f"{path}: a big-endian .ply: only binary_little_endian and ascii are read")
    if fmt not in ("binary_little_endian", "ascii"):
        raise ValueError(f"{path}: format {fmt!r}: only binary_little_endian and ascii are read")
    return fmt, elements


def load_reference_ply(path):
    """A reference scan or mesh for mesh_eval -> (points float32 [P,3], faces int32 [F,3] or None).  Reads a .ply in
    binary_little_endian or ascii format whose vertex element has x y z as float or double among any other scalar
    properties (skipped by their declared sizes) and, optionally, a face element with a list property vertex_indices or
    vertex_index of an integer type.  Refused by name (ValueError): big-endian files, a face with other than 3 corners, a
    missing x, y or z, a truncated file, a face index outside the vertices.  A file without a face element, or with zero
    faces, gives faces = None."""
    with open(path, "rb") as f:
        fmt, elements = _reference_header(f, path)
        body = f.read()
    points = faces = None
    tokens = body.split() if fmt == "ascii" else None
    pos = 0  # in bytes (binary) or tokens (ascii)
    for name, count, props in elements:
        lists = [p for p in props if p[0] == "list"]
        for p in props:
            for t in (p[1:3] if p[0] == "list" else p[:1]):
                if t not in _PLY_TYPES:
                    raise ValueError(f"{path}: element {name}: unknown property type {t!r}")
        if name == "face" and (len(lists) != 1 or lists[0][3] not in ("vertex_indices", "vertex_index")
                               or _PLY_TYPES[lists[0][2]][0] not in "iu" or _PLY_TYPES[lists[0][1]][0] not in "iu"):
            raise ValueError(f"{path}: the face element needs one list property vertex_indices (or vertex_index) of an "
                             f"integer type, got {[' '.join(p) for p in props]}")
        if name != "face" and lists:
            if points is not None and (faces is not None or not any(e[0] == "face" for e in elements)):
                break  # nothing that is read comes after it
            raise ValueError(f"{path}: element {name} has a list property and comes before the data that is read")
        # the row: scalar fields, with the face's list as a count and three indices
        fields = []
        for k, p in enumerate(props):
            if p[0] == "list":
                fields += [("_n", "<" + _PLY_TYPES[p[1]]), ("_v", "<" + _PLY_TYPES[p[2]], (3,))]
            else:
                fields.append((f"_{k}_{p[1]}" if p[1] in ("_n", "_v") else p[1], "<" + _PLY_TYPES[p[0]]))
        if len({fd[0] for fd in fields}) != len(fields):
            raise ValueError(f"{path}: element {name} declares a property twice")
        row = np.dtype(fields)
        if name == "vertex":
            missing = [c for c in "xyz" if c not in row.names]
            if missing:
                raise ValueError(f"{path}: the vertex element has no property {', '.join(missing)}")
            if any(row[c].kind != "f" for c in "xyz"):
                raise ValueError(f"{path}: x, y and z must be float or double")
        if fmt == "ascii":
            width = sum(int(np.prod(row[n].shape)) if row[n].shape else 1 for n in row.names) if row.names else 0
            chunk = tokens[pos:pos + count * width]
            if name == "face" and count:
                n_col = [n for n in row.names].index("_n")  # (scalars before the list are one token each)
                bad = len(chunk) < count * width
                try:
                    first = np.array(chunk[n_col::width], dtype=np.float64) if not bad else None
                except ValueError:
                    first = None
                if bad or first is None or not (first == 3).all():
                    j = pos  # walk the rows to name the reason
                    for _ in range(count):
                        if j + n_col >= len(tokens):
                            raise ValueError(f"{path}: truncated: element face ends early")
                        n = int(float(tokens[j + n_col]))
                        if n != 3:
                            raise ValueError(f"{path}: a face with {n} corners: only triangles are read")
                        j += width
                    raise ValueError(f"{path}: truncated: element face ends early")
            if len(chunk) < count * width:
                raise ValueError(f"{path}: truncated: element {name} ends early")
            pos += count * width
            try:
                table = np.array(chunk, dtype=np.float64).reshape(count, width)
            except ValueError:
                raise ValueError(f"{path}: element {name}: a value that is no number")
            data, col = {}, 0
            for n in row.names:
                w = 3 if row[n].shape else 1
                data[n] = table[:, col:col + w] if w == 3 else table[:, col]
                col += w
        else:
            size = count * row.itemsize
            if name == "face" and count:  # a face that is no triangle shifts every row after it: look at the counts in turn
                n_off, n_dt = row.fields["_n"][1], row.fields["_n"][0]
                whole = min(count, (len(body) - pos) // row.itemsize)
                ns = np.ndarray((whole,), dtype=n_dt, buffer=body, offset=pos + n_off, strides=(row.itemsize,)) if whole else \
                    np.zeros((0,), dtype=n_dt)
                if not (ns == 3).all():
                    raise ValueError(f"{path}: a face with {int(ns[np.nonzero(ns != 3)[0][0]])} corners: only triangles are read")
            if pos + size > len(body):
                raise ValueError(f"{path}: truncated: element {name} ends early")
            data = np.frombuffer(body, dtype=row, count=count, offset=pos)
            pos += size
        if name == "vertex":
            points = np.ascontiguousarray(np.stack([data["x"], data["y"], data["z"]], axis=1).astype(np.float32)).reshape(-1, 3)
        elif name == "face":
            idx = np.asarray(data["_v"]).reshape(-1, 3)
            if points is None:
                raise ValueError(f"{path}: the face element comes before the vertex element")
            if len(idx) and (idx.min() < 0 or idx.max() >= len(points)):
                raise ValueError(f"{path}: a face index lies outside [0, {len(points)})")
            faces = np.ascontiguousarray(idx.astype(np.int32)).reshape(-1, 3)
    if points is None:
        raise ValueError(f"{path}: no vertex element")
    return points, (faces if faces is not None and len(faces) else None)
