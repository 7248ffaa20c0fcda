"""Point-cloud batch (the PyTorch3D ``Pointclouds`` subset the point-to-mesh losses of
renderer/loss.py take): a list of (P_i,3) tensors, or a padded (N,P,3) tensor whose clouds all have
P points.

The points are kept as given, so gradients flow to the caller's tensors through every view.  The
index tables (points per cloud, first packed index, cloud of a packed point, the losses' per-point
weights) are device tensors built once and cached, like mesh._Topology's: after one call nothing is
built on the host, and a step that uses the cloud can be captured in a HIP graph.  For a padded
tensor they are filled on the device, so a cloud of fresh samples can be wrapped inside a captured
step; a list's tables are copied from the host on first use (use the cloud once before a capture)."""
import torch


class Pointclouds:
    def __init__(self, points, normals=None):
        self._padded = None
        if torch.is_tensor(points):
            if points.dim() != 3 or points.shape[2] != 3:
                raise ValueError(f"points must be (N,P,3) or a list of (P_i,3), got {tuple(points.shape)}")
            self._padded = points
            self._list = [p for p in points]
        else:
            self._list = list(points)
            for p in self._list:
                if not torch.is_tensor(p) or p.dim() != 2 or p.shape[1] != 3:
                    raise ValueError("points must be (N,P,3) or a list of (P_i,3) tensors")
            if any(p.device != self._list[0].device for p in self._list):
                raise ValueError("the clouds of a batch must be on one device")
        self._normals_padded = None
        if normals is None:
            self._normals = None
        elif torch.is_tensor(normals):
            self._normals_padded = normals
            self._normals = [n for n in normals]
        else:
            self._normals = list(normals)
        if self._normals is not None and [tuple(n.shape) for n in self._normals] != [tuple(p.shape) for p in self._list]:
            raise ValueError("normals must have the shapes of points")
        self.npoints = [p.shape[0] for p in self._list]  # Python ints: no host read later
        self.device = self._list[0].device if self._list else torch.device("cpu")
        self._idx = None
        self._weights = {}

    def __len__(self):
        return len(self._list)

    def to(self, device):
        if self._padded is not None:
            return Pointclouds(self._padded.to(device), None if self._normals is None else self.normals_padded().to(device))
        return Pointclouds([p.to(device) for p in self._list],
                           None if self._normals is None else [n.to(device) for n in self._normals])

    # ---------------------------------------------------------------- views
    def points_list(self):
        return self._list

    def points_packed(self):
        if self._padded is not None:
            return self._padded.reshape(-1, 3)
        return self._list[0] if len(self._list) == 1 else torch.cat(self._list, dim=0)

    def points_padded(self):
        return self._pad(self._list, self._padded)

    def normals_list(self):
        return self._normals

    def normals_packed(self):
        if self._normals is None:
            return None
        return self._normals[0] if len(self._normals) == 1 else torch.cat(self._normals, dim=0)

    def normals_padded(self):
        return None if self._normals is None else self._pad(self._normals, self._normals_padded)

    def _pad(self, items, padded):
        if padded is not None:
            return padded
        if len(items) == 1:
            return items[0][None]  # a view: no copy kernel
        if all(n == self.npoints[0] for n in self.npoints):
            return torch.stack(items, 0)
        out = items[0].new_zeros((len(items), max(self.npoints), 3))
        for i, p in enumerate(items):
            out[i, : p.shape[0]] = p
        return out

    # ------------------------------------------------- cached index tables
    def _tables(self):
        if self._idx is None and self._padded is not None:
            # a padded tensor: device fills only, so a cloud of fresh samples can be wrapped inside a captured step
            N, P = self._padded.shape[0], self._padded.shape[1]
            first = torch.arange(N, dtype=torch.int64, device=self.device) * P
            self._idx = dict(n=torch.full((N,), P, dtype=torch.int64, device=self.device), first=first,
                             cloud=torch.arange(N, dtype=torch.int64, device=self.device).repeat_interleave(P))
        if self._idx is None:
            n = torch.tensor(self.npoints, dtype=torch.int64)
            first = torch.cumsum(n, 0) - n
            cloud = torch.repeat_interleave(torch.arange(len(self.npoints)), n)
            self._idx = dict(n=n.to(self.device), first=first.to(self.device), cloud=cloud.to(self.device))
        return self._idx

    def num_points_per_cloud(self):
        """(N,) int64 device tensor."""
        return self._tables()["n"]

    def cloud_to_packed_first_idx(self):
        """(N,) int64: the first packed point of every cloud."""
        return self._tables()["first"]

    def packed_to_cloud_idx(self):
        """(P,) int64: the cloud of every packed point."""
        return self._tables()["cloud"]

    def loss_weights(self, dtype=torch.float32):
        """(P,) 1 / (N P_n) in `dtype`, n the packed point's cloud: the per-point weight of the
        point-to-mesh losses; not PyTorch3D API."""
        w = self._weights.get(dtype)
        if w is None and self._padded is not None:
            N, P = self._padded.shape[0], self._padded.shape[1]
            w = self._weights[dtype] = torch.full((N * P,), 1.0 / (N * max(P, 1)), dtype=dtype, device=self.device)
        if w is None:
            per = torch.tensor([1.0 / (len(self.npoints) * max(n, 1)) for n in self.npoints], dtype=torch.float64)
            w = torch.repeat_interleave(per, torch.tensor(self.npoints, dtype=torch.int64)).to(dtype)
            w = self._weights[dtype] = w.to(self.device)
        return w
