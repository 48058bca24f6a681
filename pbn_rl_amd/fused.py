"""What the two fused updates share (FusedBDQUpdate, replay.py; FusedDDQNUpdate, ddqn.py)."""
from __future__ import annotations

from typing import List

import torch

__all__ = ["FusedUpdate", "bump"]


def bump(params) -> None:
    """Mark parameters a HIP kernel rewrote in place (their version counters are how PyTorch, and
    the acting agents' pack caches, see an in-place change)."""
    for p in params:
        torch.autograd.graph.increment_version(p)


def _versions(params) -> tuple:
    return tuple(p._version for p in params)


class FusedUpdate:
    """The agent-independent half of a fused update.  Each network's parameters live in one flat fp32
    buffer (``q_flat`` / ``t_flat``) of which the module's nn.Parameters are views, so ``state_dict``,
    the PyTorch forward and the HIP kernels see the same weights; each has an image (``q_image`` /
    ``t_image``), the packed form the kernels read; Adam keeps ``m`` and ``v`` in buffers of the flat
    layout and ``step`` on the device (graph-capturable).  The kernels write parameters in place, so
    the version bookkeeping here keeps the images in step with them.

    A subclass sets the attributes its own methods read, then calls ``__init__``, and supplies:
    ``_sizes()`` -> (flat floats, image floats, workspace bytes); ``_params(module)`` -> its
    parameters as (tensor, float offset in the flat buffer) pairs in layout order;
    ``_pack(flat, image)``, the launch that builds one network's image; and ``update()``."""

    def __init__(self, q, target, net, *, batch_size: int, learning_rate: float, gamma: float, betas, eps: float,
                 keep_grad: bool):
        dev = next(q.parameters()).device
        self.net, self.N, self.B = net, net.spec.n, int(batch_size)
        self.lr, self.gamma = float(learning_rate), float(gamma)
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        self.q, self.target = q, target
        n_flat, n_image, work_bytes = self._sizes()
        self.q_flat, self.t_flat = (self._flatten(m, n_flat, dev) for m in (q, target))
        self._qp, self._tp = ([p for p, _ in self._params(m)] for m in (q, target))
        self._qv = self._tv = None
        self.m = torch.zeros_like(self.q_flat)
        self.v = torch.zeros_like(self.q_flat)
        self.step = torch.zeros(1, dtype=torch.float32, device=dev)
        self.q_image = torch.zeros(n_image, dtype=torch.float32, device=dev)
        self.t_image = torch.zeros_like(self.q_image)
        self.work = torch.empty((work_bytes + 3) // 4, dtype=torch.float32, device=dev)
        self.loss = torch.zeros(1, dtype=torch.float32, device=dev)
        self.grad = torch.zeros_like(self.q_flat) if keep_grad else None
        self.pack()

    @classmethod
    def _require_gpu(cls, q) -> None:
        if next(q.parameters()).device.type != "cuda":
            raise ValueError(f"{cls.__name__} runs on the GPU")

    def _flatten(self, module, n_flat: int, dev) -> torch.Tensor:
        flat = torch.zeros(n_flat, dtype=torch.float32, device=dev)
        with torch.no_grad():
            for p, at in self._params(module):
                view = flat[at:at + p.numel()].view(p.shape)
                view.copy_(p.detach())
                p.data = view
        return flat

    def _stream(self):
        return torch.cuda.current_stream(self.q_flat.device).cuda_stream

    def pack(self, which: str = "both") -> None:
        """Recompute the image of the online and/or target network from its flat buffer."""
        with torch.cuda.device(self.q_flat.device):
            if which in ("both", "online"):
                self._pack(self.q_flat, self.q_image)
            if which in ("both", "target"):
                self._pack(self.t_flat, self.t_image)
        if which in ("both", "online"):
            self._qv = _versions(self._qp)
        if which in ("both", "target"):
            self._tv = _versions(self._tp)

    def sync(self) -> None:
        """Repack the image of a network whose parameters changed since its last pack (e.g. a
        load_state_dict: the copy bumps the parameters' versions); a no-op otherwise."""
        if _versions(self._qp) != self._qv:
            self.pack("online")
        if _versions(self._tp) != self._tv:
            self.pack("target")

    def mark_updated(self) -> None:
        """After an update's launches (eager, or a replayed graph holding them): the online
        parameters changed in place, and the launches rewrote the online image with them."""
        bump(self._qp)
        self._qv = _versions(self._qp)

    def mark_target_updated(self) -> None:
        """After launches that rewrote the target's parameters in place and its image with them."""
        bump(self._tp)
        self._tv = _versions(self._tp)

    # the buffers a checkpoint holds (FusedDDQNUpdate adds grad_norm).  The images and the workspace
    # are derived: pack() reproduces bit for bit the images an update leaves
    _STATE_TENSORS = ("q_flat", "t_flat", "m", "v", "step", "loss")

    def state_dict(self) -> dict:
        return {k: getattr(self, k).detach().to("cpu", copy=True) for k in self._STATE_TENSORS}

    def load_state_dict(self, sd: dict) -> None:
        """In place into the flat buffers (the nn.Parameters are views of them); then both images are
        rebuilt and both networks marked as changed."""
        with torch.no_grad():
            for k in self._STATE_TENSORS:
                getattr(self, k).copy_(sd[k])
        self.pack("both")
        self.mark_updated()
        self.mark_target_updated()

    def _check_idx(self, idx: torch.Tensor) -> None:
        if idx.shape != (self.B,) or idx.dtype != torch.int64:
            raise ValueError(f"idx must be {self.B} int64 ring indices")

    @staticmethod
    def check_per_args(B: int, device, weights, priorities_out) -> None:
        """update()'s importance-weight arguments: both or neither, contiguous float32 [B] tensors
        on ``device``.  Raises ValueError naming the offending argument."""
        if weights is None:
            if priorities_out is not None:
                raise ValueError("priorities_out needs weights")
            return
        if priorities_out is None:
            raise ValueError("priorities_out is required with weights")
        for name, t in (("weights", weights), ("priorities_out", priorities_out)):
            if (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.shape != (B,)
                    or not t.is_contiguous() or t.device != torch.device(device)):
                raise ValueError(f"{name} must be a contiguous float32 [{B}] tensor on {device}")

    def grads(self) -> List[torch.Tensor]:
        """The last update's clipped gradient (keep_grad=True) as views shaped like q.parameters()."""
        if self.grad is None:
            raise ValueError("construct with keep_grad=True")
        g = {id(p): self.grad[at:at + p.numel()].view(p.shape) for p, at in self._params(self.q)}
        return [g[id(p)] for p in self.q.parameters()]
