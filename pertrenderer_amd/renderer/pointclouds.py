"""Point-cloud batch (the PyTorch3D ``Pointclouds`` subset the point-to-mesh losses of
renderer/loss.py and the point renderer of renderer/points.py take): a list of (P_i,3) tensors, or a
padded (N,P,3) tensor whose clouds all have P points, with optional normals and per-point features
(C channels, the colours PointsRenderer composites) in the same two forms.

The points are kept as given, so gradients flow to the caller's tensors through every view.  The
index tables (points per cloud, first packed index, cloud of a packed point, the losses' per-point
weights) are device tensors built once and cached, like mesh._Topology's: after one call nothing is
built on the host, and a step that uses the cloud can be captured in a HIP graph.  For a padded
tensor they are filled on the device, so a cloud of fresh samples can be wrapped inside a captured
step; a list's tables are copied from the host on first use (use the cloud once before a capture)."""
import torch


class Pointclouds:
    def __init__(self, points, normals=None, features=None):
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
        # per-point features (colours, ...) of C channels: a list of (P_i,C) or a padded (N,P,C) tensor
        self._features_padded = None
        if features is None:
            self._features = None
        elif torch.is_tensor(features):
            if features.dim() != 3:
                raise ValueError(f"features must be (N,P,C) or a list of (P_i,C), got {tuple(features.shape)}")
            self._features_padded = features
            self._features = [f for f in features]
        else:
            self._features = list(features)
        if self._features is not None:
            if (len(self._features) != len(self._list)
                    or any(not torch.is_tensor(f) or f.dim() != 2 for f in self._features)
                    or [f.shape[0] for f in self._features] != self.npoints
                    or any(f.shape[1] != self._features[0].shape[1] for f in self._features)):
                raise ValueError("features must have one (P_i,C) row block per cloud, with one C")
        self.device = self._list[0].device if self._list else torch.device("cpu")
        self._idx = None
        self._weights = {}

    def __len__(self):
        return len(self._list)

    def to(self, device):
        if self._padded is not None:
            return Pointclouds(self._padded.to(device), None if self._normals is None else self.normals_padded().to(device),
                               None if self._features is None else self.features_padded().to(device))
        return Pointclouds([p.to(device) for p in self._list],
                           None if self._normals is None else [n.to(device) for n in self._normals],
                           None if self._features is None else [f.to(device) for f in self._features])

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

    def features_list(self):
        return self._features

    def features_packed(self):
        """(P,C) rows in packed order (one point's channels are contiguous), or None."""
        if self._features is None:
            return None
        if self._features_padded is not None:
            return self._features_padded.reshape(-1, self._features_padded.shape[2])
        return self._features[0] if len(self._features) == 1 else torch.cat(self._features, dim=0)

    def features_padded(self):
        return None if self._features is None else self._pad(self._features, self._features_padded)

    def update_padded(self, new_points):
        """A cloud batch with the points `new_points` (N,P,3) (P the longest cloud; rows past a cloud's
        count are dropped) and this batch's features, normals and cached index tables."""
        if not torch.is_tensor(new_points) or tuple(new_points.shape) != (len(self._list), max(self.npoints, default=0), 3):
            raise ValueError(f"new_points must be ({len(self._list)},{max(self.npoints, default=0)},3)")
        if self._padded is not None:
            return self._with_points(new_points)
        return self._with_points([new_points[i, :n] for i, n in enumerate(self.npoints)])

    def _with_points(self, points):
        """This batch with other points of the same sizes (a padded tensor or a list)."""
        new = Pointclouds(points)
        if new.npoints != self.npoints:
            raise ValueError(f"the new points must have {self.npoints} rows per cloud, got {new.npoints}")
        new._normals, new._normals_padded = self._normals, self._normals_padded
        new._features, new._features_padded = self._features, self._features_padded
        new._idx, new._weights = self._idx, self._weights
        return new

    def _pad(self, items, padded):
        if padded is not None:
            return padded
        if len(items) == 1:
            return items[0][None]  # a view: no copy kernel
        if all(n == self.npoints[0] for n in self.npoints):
            return torch.stack(items, 0)
        out = items[0].new_zeros((len(items), max(self.npoints), items[0].shape[1]))
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
