"""Depth encoder and height-scan distiller (project-only: the reference has no depth sensor).

``DepthEncoder`` is a small CNN over the egocentric depth image (``env.depth_images``): three strided convolutions, two
dense layers, ELU.  Its parameters are views of one flat buffer, so the native path (csrc/lrl_vision.hip: the whole conv
stack as one launch per direction, the dense layers on the GEMM families) and ``torch.optim.Adam`` see the same storage.
``DepthDistiller`` regresses the privileged height scan at the end of ``obs`` from the image and the proprioceptive
columns, so that a perceptive policy can act on what a real robot measures.
"""
import ctypes as C
import os

import torch
from torch import nn
from torch.nn import functional as F

from . import _abi

MAX_WORKGROUPS = 512  # LRL_VISION_MAX_WORKGROUPS
_HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "include",
                       "lrl_vision.h")
_lib = None


def lib():
    """liblrl.so with the lrl_vision_* entry points typed from include/lrl_vision.h (the header include/lrl.h pulls
    in; _abi.lib() types the functions lrl.h itself declares).  lrl_vision_net is not one of _abi.MIRRORS, so a
    pointer to it is a c_void_p: callers pass ``ctypes.addressof``."""
    global _lib
    if _lib is None:
        L = _abi.lib()
        with open(_HEADER) as f:
            for name, (restype, argtypes) in _abi.signatures(f.read()).items():
                fn = getattr(L, name)
                fn.restype, fn.argtypes = restype, argtypes
        _lib = L
    return _lib


class LrlVisionNet(C.Structure):
    """lrl_vision_net (include/lrl_vision.h).  Not one of _abi.MIRRORS: the entry points take it as a plain address
    (``ctypes.addressof``); tests/test_vision.py pins the layout with a compiled probe."""
    _fields_ = [(k, C.c_int32) for k in ("height", "width", "extra", "hidden", "out")] + \
               [("input_scale", C.c_float), ("features", C.c_int32), ("ld_x", C.c_int32)] + \
               [(k, C.c_int64) for k in ("c1w", "c1b", "c2w", "c2b", "c3w", "c3b", "f1w", "f1b", "f2w", "f2b", "total")]


_FIELDS = (("conv1.weight", "c1w"), ("conv1.bias", "c1b"), ("conv2.weight", "c2w"), ("conv2.bias", "c2b"),
           ("conv3.weight", "c3w"), ("conv3.bias", "c3b"), ("fc1.weight", "f1w"), ("fc1.bias", "f1b"),
           ("fc2.weight", "f2w"), ("fc2.bias", "f2b"))


def in_envelope(height, width, extra_dim, hidden, out_dim):
    """The sizes lrl_vision_net_init accepts (include/lrl_vision.h)."""
    return (height >= 16 and width >= 16 and height % 8 == 0 and width % 8 == 0 and height * width <= 3072 and
            16 <= hidden <= 256 and hidden % 16 == 0 and 1 <= out_dim <= 256 and 0 <= extra_dim <= 256)


def field_offsets(height, width, extra_dim, hidden, out_dim):
    """{state_dict key: (offset, shape)} and the buffer length: the fields in state_dict order, each aligned to 64
    floats (what lrl_vision_net_init computes, for any sizes)."""
    feat = 32 * (height // 8) * (width // 8)
    shapes = {"conv1.weight": (16, 1, 5, 5), "conv1.bias": (16,), "conv2.weight": (32, 16, 3, 3), "conv2.bias": (32,),
              "conv3.weight": (32, 32, 3, 3), "conv3.bias": (32,), "fc1.weight": (hidden, feat + extra_dim),
              "fc1.bias": (hidden,), "fc2.weight": (out_dim, hidden), "fc2.bias": (out_dim,)}
    out, off = {}, 0
    for key, _ in _FIELDS:
        off = (off + 63) // 64 * 64
        out[key] = (off, shapes[key])
        n = 1
        for s in shapes[key]:
            n *= s
        off += n
    return out, (off + 63) // 64 * 64


class DepthEncoder(nn.Module):
    """depth image [N, H, W] (metres) and ``extra`` [N, extra_dim] -> [N, out_dim].

    x = depth / far; conv1 1->16 5x5 s2 p2; conv2 16->32 3x3 s2 p1; conv3 32->32 3x3 s2 p1 (ELU after each);
    flatten; concatenate extra; fc1 -> hidden, ELU; fc2 -> out_dim.  ``forward`` is the torch form with autograd (CPU,
    sizes outside the native envelope, comparisons); ``forward_native`` / ``mse_backward_native`` run liblrl's kernels
    and leave the gradient in ``flat.grad``."""

    def __init__(self, height, width, out_dim, extra_dim=0, hidden=128, far=3.0):
        super().__init__()
        if height % 8 or width % 8 or height < 8 or width < 8:
            raise ValueError(f"DepthEncoder: height and width must be multiples of 8, got {height} x {width}")
        self.height, self.width, self.out_dim, self.extra_dim, self.hidden = height, width, out_dim, extra_dim, hidden
        self.far = float(far)
        self.input_scale = 1.0 / self.far
        self.features = 32 * (height // 8) * (width // 8)
        self.conv1 = nn.Conv2d(1, 16, 5, stride=2, padding=2)
        self.conv2 = nn.Conv2d(16, 32, 3, stride=2, padding=1)
        self.conv3 = nn.Conv2d(32, 32, 3, stride=2, padding=1)
        self.fc1 = nn.Linear(self.features + extra_dim, hidden)
        self.fc2 = nn.Linear(hidden, out_dim)
        self.native_ok = in_envelope(height, width, extra_dim, hidden, out_dim)
        self._net = None
        self._ws = None
        self.flatten_parameters()

    # ---- the flat buffer ----
    def flatten_parameters(self):
        """Move every parameter into one flat fp32 buffer on its current device, as views (state_dict order, 64-float
        aligned fields); ``self.flat`` is the buffer, a leaf whose ``.grad`` the parameters' ``.grad`` are views of."""
        offs, total = field_offsets(self.height, self.width, self.extra_dim, self.hidden, self.out_dim)
        named = dict(self.named_parameters())
        dev, dtype = named["conv1.weight"].device, named["conv1.weight"].dtype
        flat = torch.zeros(total, device=dev, dtype=dtype)
        with torch.no_grad():
            for key, (off, shape) in offs.items():
                p = named[key]
                n = p.numel()
                flat[off:off + n].copy_(p.detach().reshape(-1))
                p.data = flat[off:off + n].view(shape)
        flat.grad = torch.zeros_like(flat)
        self.flat, self.flat_grad, self.offsets = flat, flat.grad, offs
        self._attach_grads()
        self._ws = None
        return flat

    def _attach_grads(self):
        """Every parameter's .grad is its view of ``flat.grad`` (again, after an optimiser's zero_grad dropped it)."""
        for key, p in self.named_parameters():
            off, shape = self.offsets[key]
            if p.grad is None or p.grad.data_ptr() != self.flat_grad.data_ptr() + off * self.flat_grad.element_size():
                p.grad = self.flat_grad[off:off + p.numel()].view(shape)

    def _apply(self, fn, *a, **kw):
        out = super()._apply(fn, *a, **kw)
        self.flatten_parameters()  # (a move to another device copies tensor by tensor: make them views again)
        return out

    def zero_grad(self, set_to_none=False):
        self.flat_grad.zero_()
        self._attach_grads()

    # ---- torch form ----
    def forward(self, images, extra=None):
        x = images.unsqueeze(1) * self.input_scale
        x = F.elu(self.conv1(x))
        x = F.elu(self.conv2(x))
        x = F.elu(self.conv3(x))
        x = x.flatten(1)
        if self.extra_dim:
            x = torch.cat([x, extra], 1)
        return self.fc2(F.elu(self.fc1(x)))

    def conv_features(self, images):
        x = images.unsqueeze(1) * self.input_scale
        return F.elu(self.conv3(F.elu(self.conv2(F.elu(self.conv1(x)))))).flatten(1)

    # ---- native form ----
    def net(self):
        """The lrl_vision_net descriptor (lrl_vision_net_init); raises outside the envelope."""
        if self._net is None:
            n = LrlVisionNet()
            _abi.check(lib().lrl_vision_net_init(C.addressof(n), self.height, self.width, self.extra_dim,
                                                      self.hidden, self.out_dim, self.input_scale))
            for key, name in _FIELDS:
                assert getattr(n, name) == self.offsets[key][0], key
            assert n.total == self.flat.numel()
            self._net = n
        return self._net

    def _workspace(self, batch):
        ws = self._ws
        need = lib().lrl_vision_workspace_bytes(C.addressof(self.net()), batch)
        if ws is None or ws.numel() < need or ws.device != self.flat.device:
            ws = self._ws = torch.empty(need, dtype=torch.uint8, device=self.flat.device)
        return ws

    def _check(self, images, extra, rows):
        if not self.native_ok:
            raise RuntimeError("DepthEncoder: sizes outside the native envelope (include/lrl_vision.h); use forward()")
        if not images.is_cuda or images.dtype != torch.float32 or not images.is_contiguous() or \
                tuple(images.shape[1:]) != (self.height, self.width):
            raise ValueError("DepthEncoder: images must be a contiguous float32 device tensor [N, H, W]")
        if self.extra_dim:
            if extra is None or extra.dim() != 2 or extra.shape[1] < self.extra_dim or extra.stride(1) != 1 or \
                    extra.dtype != torch.float32 or extra.device != images.device:
                raise ValueError("DepthEncoder: extra must be float32 [N, >= extra_dim] with unit column stride")
        if rows is not None and (rows.dtype != torch.int64 or not rows.is_contiguous()):
            raise ValueError("DepthEncoder: rows must be a contiguous int64 tensor")
        return int(rows.numel()) if rows is not None else int(images.shape[0])

    def forward_native(self, images, extra=None, rows=None, features=None):
        """The network's output [batch, out_dim] from liblrl (no autograd).  ``rows`` (int64) picks the samples; a
        float32 ``features`` tensor [batch, F] receives the conv stack's output."""
        batch = self._check(images, extra, rows)
        out = torch.empty(batch, self.out_dim, device=images.device)
        ws = self._workspace(batch)
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        _abi.check(lib().lrl_vision_forward(
            C.addressof(self.net()), p(self.flat), p(images), p(extra) if self.extra_dim else None,
            extra.stride(0) if self.extra_dim else 0, p(rows), batch, p(out), p(features), p(ws),
            _abi.stream_of(str(images.device))))
        return out

    def mse_backward_native(self, images, extra, target, rows=None):
        """mean((net(images, extra) - target)^2) and its gradient, written into ``flat_grad`` (the parameters' .grad);
        returns the loss as a float64 device scalar."""
        batch = self._check(images, extra, rows)
        if target.dim() != 2 or target.shape[1] < self.out_dim or target.stride(1) != 1 or target.dtype != torch.float32:
            raise ValueError("DepthEncoder: target must be float32 [N, >= out_dim] with unit column stride")
        loss = torch.empty((), dtype=torch.float64, device=images.device)
        self._attach_grads()
        ws = self._workspace(batch)
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        _abi.check(lib().lrl_vision_forward_backward(
            C.addressof(self.net()), p(self.flat), p(self.flat_grad), p(images), p(extra) if self.extra_dim else None,
            extra.stride(0) if self.extra_dim else 0, p(target), target.stride(0), p(rows), batch, p(loss), p(ws),
            _abi.stream_of(str(images.device))))
        return loss


def scan_columns(env):
    """(first scan column, number of scan columns) of ``obs``: the height scan is the row's tail."""
    n = int(env.cfg.env.num_height_points) if env.cfg.terrain.measure_heights else 0
    if n <= 0:
        raise ValueError("DepthDistiller: the env has no height scan (cfg.terrain.measure_heights)")
    return int(env.cfg.env.num_observations) - n, n


class DepthDistiller:
    """Regress the height-scan columns of ``obs`` from the depth image and the other columns.

    ``collect(obs)`` after a step whose ``env.depth_refreshed`` is True appends every env's (image, extra, target) to
    device rings of ``capacity`` rows; ``update(n)`` runs n Adam steps on random minibatches (the rings are read in
    place through ``rows``); ``predict_obs(obs)`` swaps the scan columns for the encoder's output.  It reads from the
    env and writes nothing to it.  ``sensed=True``: ``collect`` and ``predict_obs`` read ``env.depth_sensed``, the
    sensor model's noisy, late images (lrl.config.add_depth_sensor), and an env without it is refused."""

    def __init__(self, env, encoder, capacity=16384, batch_size=1024, lr=1e-3, native=None, seed=0, sensed=False):
        self.env, self.encoder = env, encoder
        # sensed: read env.depth_sensed (the sensor model's images, Cfg.depth_sensor) in place of the exact ones
        self.sensed = bool(sensed)
        if self.sensed and getattr(env, "depth_sensed", None) is None:
            raise ValueError("DepthDistiller(sensed=True): the env has no depth sensor model (the cfg has no "
                             "depth_sensor group, lrl.config.add_depth_sensor)")
        self.first, self.num_scan = scan_columns(env)
        if encoder.out_dim != self.num_scan or encoder.extra_dim != self.first:
            raise ValueError(f"DepthDistiller: the encoder maps {encoder.extra_dim} extra columns to {encoder.out_dim}, "
                             f"the env's obs has {self.first} + {self.num_scan}")
        h, w = env.depth_images.shape[1:]
        if (h, w) != (encoder.height, encoder.width):
            raise ValueError(f"DepthDistiller: the encoder takes {encoder.height} x {encoder.width} images, the camera "
                             f"draws {h} x {w}")
        dev = env.depth_images.device
        self.capacity, self.batch_size = int(capacity), int(batch_size)
        self.images = torch.zeros(self.capacity, h, w, device=dev)
        self.obs = torch.zeros(self.capacity, self.first + self.num_scan, device=dev)  # extra | target in one row
        self.extra, self.target = self.obs[:, :self.first], self.obs[:, self.first:]
        self.head, self.size = 0, 0
        self.native = (encoder.native_ok and dev.type == "cuda") if native is None else bool(native)
        self.optimizer = torch.optim.Adam(encoder.parameters(), lr=lr)
        self.gen = torch.Generator(device=dev)
        self.gen.manual_seed(seed)

    def _env_images(self):
        return self.env.depth_sensed if self.sensed else self.env.depth_images

    def collect(self, obs, env_ids=None):
        """Append (depth image, extra, target) of every env (or of ``env_ids``) at the ring's head, wrapping."""
        img = self._env_images()
        if env_ids is not None:
            img, obs = img[env_ids], obs[env_ids]
        n = img.shape[0]
        if n > self.capacity:
            raise ValueError(f"DepthDistiller: {n} rows do not fit a ring of {self.capacity}")
        first = min(n, self.capacity - self.head)
        self.images[self.head:self.head + first].copy_(img[:first])
        self.obs[self.head:self.head + first].copy_(obs[:first])
        if first < n:
            self.images[:n - first].copy_(img[first:])
            self.obs[:n - first].copy_(obs[first:])
        self.head = (self.head + n) % self.capacity
        self.size = min(self.size + n, self.capacity)

    def loss_on(self, rows):
        """Loss and gradient (into the parameters' .grad) of the minibatch ``rows`` of the rings."""
        enc = self.encoder
        if self.native:
            return enc.mse_backward_native(self.images, self.extra, self.target, rows)
        enc.zero_grad()
        loss = F.mse_loss(enc(self.images[rows], self.extra[rows]), self.target[rows])
        loss.backward()
        return loss.detach().double()

    def update(self, n=1, rows=None):
        """n Adam steps on random minibatches of the collected rows (``rows``: a list of n index tensors instead).
        Returns the mean loss as a device scalar; nothing in the loop waits for the device."""
        if self.size == 0:
            raise RuntimeError("DepthDistiller.update: nothing collected")
        dev = self.images.device
        total = torch.zeros((), dtype=torch.float64, device=dev)
        for i in range(n):
            r = rows[i] if rows is not None else \
                torch.randint(self.size, (min(self.batch_size, self.size),), device=dev, generator=self.gen)
            total += self.loss_on(r)
            self.optimizer.step()
        return total / n

    @torch.no_grad()
    def evaluate(self, images, obs):
        """MSE of the encoder on given images / obs rows (a held-out set), a device scalar."""
        extra, target = obs[:, :self.first], obs[:, self.first:]
        pred = self.encoder.forward_native(images, extra) if self.native else self.encoder(images, extra)
        return F.mse_loss(pred, target)

    @torch.no_grad()
    def predict_obs(self, obs):
        """``obs`` with its scan columns replaced by the encoder's output from the env's current depth images."""
        extra = obs[:, :self.first]
        img = self._env_images()
        pred = self.encoder.forward_native(img, extra) if self.native else self.encoder(img, extra)
        out = obs.clone()
        out[:, self.first:] = pred
        return out
