"""The topology caches of the mesh regularisers (_Topology.edges_packed / neighbour_csr /
face_pairs, renderer/mesh.py) against brute-force Python sets, on CPU."""
import pytest
import torch

from mesh_loss_cases import TOPOLOGY_CASES, brute_edges, case, packed
from pertrenderer_amd.renderer import Meshes


def _mesh(name):
    verts, faces = case(name)
    return Meshes([v.clone() for v in verts], [f.clone() for f in faces]), verts, faces


@pytest.mark.parametrize("name", TOPOLOGY_CASES)
def test_edges_packed_matches_brute_force(name):
    m, verts, faces = _mesh(name)
    _, f = packed(verts, faces)
    e = m.edges_packed()
    assert e.dtype == torch.int64 and e.shape[1] == 2
    assert e.tolist() == [list(x) for x in brute_edges(f)]  # unique, a < b, lexicographic
    assert bool((e[:, 0] < e[:, 1]).all())
    # per-mesh counts: every edge belongs to the mesh of its vertices
    first = [0]
    for v in verts:
        first.append(first[-1] + v.shape[0])
    want = [sum(1 for a, _ in brute_edges(f) if first[i] <= a < first[i + 1]) for i in range(len(verts))]
    n = m.num_edges_per_mesh()
    assert torch.is_tensor(n) and n.dtype == torch.int64 and n.tolist() == want


@pytest.mark.parametrize("name", TOPOLOGY_CASES)
def test_neighbour_csr_matches_brute_force(name):
    m, verts, faces = _mesh(name)
    v, f = packed(verts, faces)
    nbrs = [set() for _ in range(v.shape[0])]
    for a, b in brute_edges(f):
        nbrs[a].add(b)
        nbrs[b].add(a)
    start, nbr = m.neighbour_csr()
    assert start.dtype == nbr.dtype == torch.int64
    assert start.shape[0] == v.shape[0] + 1 and nbr.shape[0] == 2 * len(brute_edges(f))
    for i, s in enumerate(nbrs):
        assert nbr[start[i]:start[i + 1]].tolist() == sorted(s), i
    if name == "isolated":
        assert start[-1] == start[-2]  # the isolated vertex has an empty row


def _pairs_by_sort(v, f):
    """mesh_normal_consistency's per-call derivation, as it stood before the cache."""
    e = torch.cat([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 0).sort(dim=1).values
    fid = torch.arange(f.shape[0]).repeat(3)
    key = e[:, 0] * (v.shape[0] + 1) + e[:, 1]
    order = key.argsort()
    k, fo = key[order], fid[order]
    same = k[1:] == k[:-1]
    return fo[:-1][same], fo[1:][same]


@pytest.mark.parametrize("name", TOPOLOGY_CASES)
def test_face_pairs_match_the_per_call_sort(name):
    m, verts, faces = _mesh(name)
    v, f = packed(verts, faces)
    a, b, n = m.face_pairs()
    wa, wb = _pairs_by_sort(v, f)
    assert isinstance(n, int) and n == wa.shape[0]
    assert torch.equal(a, wa) and torch.equal(b, wb)
    # and against sets: an edge shared by k faces gives k - 1 pairs of faces that do share it
    count = {}
    for fi, (x, y, z) in enumerate(f.tolist()):
        for p, q in ((x, y), (y, z), (z, x)):
            count.setdefault((min(p, q), max(p, q)), []).append(fi)
    assert n == sum(len(c) - 1 for c in count.values())
    shared = {frozenset((p, q)) for c in count.values() for p in c for q in c if p != q}
    assert all(frozenset(pq) in shared for pq in zip(a.tolist(), b.tolist()))
    if name == "triangle":
        assert n == 0
    if name == "fan3":
        assert n == 2


def test_derived_meshes_share_the_caches():
    m, verts, _ = _mesh("batch2")
    caches = (m.edges_packed(), m.num_edges_per_mesh(), *m.neighbour_csr(), *m.face_pairs())
    d = m.offset_verts(torch.full((sum(v.shape[0] for v in verts), 3), 0.25))
    got = (d.edges_packed(), d.num_edges_per_mesh(), *d.neighbour_csr(), *d.face_pairs())
    assert all(x is y for x, y in zip(caches, got))
    u = m.update_padded(m.verts_padded() * 2.0)
    assert u.edges_packed() is caches[0] and u.neighbour_csr()[1] is caches[3]
