"""numpy restatement of the mesh cleanup contract ("Mesh cleanup"), written from the contract and not
from csrc/mesh.hip: two vertices are connected when a face names both; label[v] is the smallest vertex index of v's
component (v for a vertex no face names); a component's size is the number of faces whose first vertex carries its label;
a component is kept iff size >= max(min_faces, 1) and, with keep_largest = K > 0, its rank among ALL components (size
descending, then label ascending) is below K; kept vertices are exactly those a kept face names; order is preserved."""
import numpy as np


def labels(faces, V):
    """Union-find with path halving, the smaller root the parent of the larger: the root of a set is its minimum."""
    parent = list(range(V))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b, c in np.asarray(faces, dtype=np.int64).reshape(-1, 3).tolist():
        for u, v in ((a, b), (a, c)):
            ru, rv = find(u), find(v)
            if ru < rv:
                parent[rv] = ru
            elif rv < ru:
                parent[ru] = rv
    return np.array([find(v) for v in range(V)], dtype=np.int32).reshape(V)


def sizes(faces, lab):
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    return np.bincount(lab[faces[:, 0]], minlength=len(lab)).astype(np.int32)


def kept_labels(count, min_faces=0, keep_largest=0):
    """-> (the labels of all components with a face, ascending; those the rule keeps, ascending)."""
    comp = np.nonzero(count)[0]
    size = count[comp].astype(np.int64)
    keep = size >= max(int(min_faces), 1)
    if keep_largest > 0:
        order = np.lexsort((comp, -size))  # primary: size descending; then label ascending
        rank = np.empty(len(comp), dtype=np.int64)
        rank[order] = np.arange(len(comp))
        keep &= rank < keep_largest
    return comp, comp[keep]


def clean(verts, colours, faces, min_faces=0, keep_largest=0):
    """-> (verts, colours, faces, report) as clm_gs_amd.mesh_clean.clean, without `rounds` in the report."""
    verts, colours = np.asarray(verts), np.asarray(colours)
    faces = np.asarray(faces, dtype=np.int32).reshape(-1, 3)
    V = len(verts)
    lab = labels(faces, V)
    count = sizes(faces, lab)
    comp, kept = kept_labels(count, min_faces, keep_largest)
    keep_label = np.zeros(V, dtype=bool)
    keep_label[kept] = True
    f = faces[keep_label[lab[faces[:, 0]]]] if len(faces) else faces
    keep_vert = np.zeros(V, dtype=bool)
    keep_vert[f.reshape(-1)] = True
    remap = np.cumsum(keep_vert) - 1
    nf = remap[f].astype(np.int32).reshape(-1, 3)
    report = dict(components=len(comp), components_kept=len(kept), vertices_removed=V - int(keep_vert.sum()),
                  faces_removed=len(faces) - len(nf), largest_faces=int(count.max()) if len(comp) else 0)
    return verts[keep_vert], colours[keep_vert], nf, report


def bfs_labels(faces, V):
    """Brute force: breadth-first search over the vertex adjacency the faces define."""
    adj = [set() for _ in range(V)]
    for a, b, c in np.asarray(faces, dtype=np.int64).reshape(-1, 3).tolist():
        for u, v in ((a, b), (b, c), (c, a)):
            adj[u].add(v)
            adj[v].add(u)
    lab = [-1] * V
    for s in range(V):  # ascending: the first vertex to reach a component is its minimum
        if lab[s] >= 0:
            continue
        lab[s], todo = s, [s]
        while todo:
            nxt = []
            for u in todo:
                for v in adj[u]:
                    if lab[v] < 0:
                        lab[v] = s
                        nxt.append(v)
            todo = nxt
    return np.array(lab, dtype=np.int32).reshape(V)
