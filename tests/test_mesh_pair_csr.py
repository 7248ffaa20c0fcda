"""_Topology.face_pair_csr (renderer/mesh.py), the face -> partner-faces CSR the native normal
consistency gathers over, against a brute-force Python construction from face_pairs(), on CPU."""
import pytest
import torch

from mesh_loss_cases import TOPOLOGY_CASES, case
from pertrenderer_amd.renderer import Meshes


def _mesh(name):
    verts, faces = case(name)
    return Meshes([v.clone() for v in verts], [f.clone() for f in faces])


@pytest.mark.parametrize("name", TOPOLOGY_CASES)
def test_face_pair_csr_matches_brute_force(name):
    m = _mesh(name)
    a, b, n = m.face_pairs()
    F = m.faces_packed().shape[0]
    rows = [[] for _ in range(F)]
    for x, y in zip(a.tolist(), b.tolist()):  # in pair order: a row is in ascending pair index
        rows[x].append(y)
        rows[y].append(x)
    start, partner = m._topo.face_pair_csr()
    assert start.dtype == partner.dtype == torch.int64
    assert start.shape == (F + 1,) and partner.shape == (2 * n,)
    assert start[0] == 0 and start[-1] == 2 * n
    for f, want in enumerate(rows):
        assert partner[start[f]:start[f + 1]].tolist() == want, f
    if name == "triangle":  # no pairs: every row empty
        assert n == 0 and start.tolist() == [0, 0]
    if name == "fan3":  # three faces on edge (0,1): two pairs, the middle face of the sort in both
        assert n == 2 and sorted((start[1:] - start[:-1]).tolist()) == [1, 1, 2]


def test_face_pair_csr_is_cached_and_shared_by_derived_meshes():
    m = _mesh("batch2")
    pairs = m.face_pairs()
    csr = m._topo.face_pair_csr()
    assert all(x is y for x, y in zip(csr, m._topo.face_pair_csr()))
    assert all(x is y for x, y in zip(pairs, m.face_pairs()))  # building the CSR leaves the pairs alone
    d = m.offset_verts(torch.full((m.verts_packed().shape[0], 3), 0.25))
    u = m.update_padded(m.verts_padded() * 2.0)
    for other in (d, u):
        assert all(x is y for x, y in zip(csr, other._topo.face_pair_csr()))
