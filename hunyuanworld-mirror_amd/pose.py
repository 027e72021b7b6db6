"""Per-image camera-pose corrections for the post-3DGS optimisation: the ``CameraOptModule`` of the reference trainer
(``--pose_opt`` / ``--pose_noise``, simple_trainer_worldmirror.py:511-523; gsplat examples/utils.py), written from its description.

Nine numbers per image: a translation delta and a rotation delta in the continuous 6-D representation (Zhou et al., "On the
Continuity of Rotation Representations in Neural Networks", CVPR 2019).  The correction multiplies into ``camtoworlds`` from the
right before every render; trained on the camera gradient of ``Rasterizer(camera_grad=True)``.  Plain torch: a few 3-vectors per
image, nothing for a kernel to do.  ``state_dict()`` has ``embeds.weight`` [n,9] and ``identity`` [6], so the ``pose_adjust`` entry
of a trainer checkpoint loads as it is."""
from __future__ import annotations

import torch
import torch.nn.functional as F


def rotation_from_6d(d6: torch.Tensor) -> torch.Tensor:
    """[...,6] -> rotation matrices [...,3,3]: Gram-Schmidt on the two 3-vectors (rows 0 and 1), row 2 their cross product"""
    a1, a2 = d6[..., :3], d6[..., 3:]
    r0 = F.normalize(a1, dim=-1)
    r1 = F.normalize(a2 - (r0 * a2).sum(-1, keepdim=True) * r0, dim=-1)
    return torch.stack((r0, r1, torch.linalg.cross(r0, r1, dim=-1)), dim=-2)


class CameraOptModule(torch.nn.Module):
    def __init__(self, n: int):
        super().__init__()
        self.embeds = torch.nn.Embedding(n, 9)      # per image: translation delta 3 | 6-D rotation delta
        self.register_buffer("identity", torch.tensor([1.0, 0.0, 0.0, 0.0, 1.0, 0.0]))   # the identity rotation in 6-D

    def zero_init(self):
        torch.nn.init.zeros_(self.embeds.weight)

    def random_init(self, std: float):
        torch.nn.init.normal_(self.embeds.weight, std=std)

    def forward(self, camtoworlds: torch.Tensor, embed_ids: torch.Tensor) -> torch.Tensor:
        """camtoworlds [...,4,4], embed_ids [...] -> camtoworlds @ [[R(6-D delta + identity), dx], [0 0 0 1]]"""
        if camtoworlds.shape[:-2] != embed_ids.shape:
            raise ValueError(f"one embed id per pose: camtoworlds {tuple(camtoworlds.shape)}, embed_ids {tuple(embed_ids.shape)}")
        delta = self.embeds(embed_ids)
        top = torch.cat((rotation_from_6d(delta[..., 3:] + self.identity), delta[..., :3, None]), dim=-1)      # [...,3,4]
        bottom = top.new_tensor([0.0, 0.0, 0.0, 1.0]).expand(*top.shape[:-2], 1, 4)
        return camtoworlds @ torch.cat((top, bottom), dim=-2)
