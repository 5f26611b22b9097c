"""``Handle`` -- what every Python class around a handle of the C ABI shares: the loaded library, the handle and its lifetime,
the HIP stream of a call, and the checks of the torch tensors whose pointers are handed over."""
from __future__ import annotations

import ctypes as C
import weakref

from . import _abi


class Handle:
    """A subclass names the ABI's destroy function in ``_destroy``, sets ``device`` and opens its handle with ``_create``
    (into ``_h``).  A handle bound to another one (a task layer to its simulator) passes it as ``parent``: the C side's destroy of the child
    dereferences the parent, so a parent is never destroyed while a child is open.  The child holds the parent (dropping references
    destroys the child first), the parent knows its children weakly (``close()`` closes them first) and counts the open ones."""

    _destroy: str = ""
    _h = None
    _parent = None
    _children = ()
    _open_children = 0
    _close_pending = False

    def __init__(self, device: int = 0, parent=None):
        self._lib = _abi.load_library()
        self.device = int(device)
        if parent is not None:
            if not parent._h:
                raise ValueError(f"{type(parent).__name__} is closed: nothing can be bound to it")
            parent._children = [r for r in parent._children if r() is not None] + [weakref.ref(self)]
            parent._open_children += 1
            self._parent = parent

    # -- lifetime ---------------------------------------------------------------------------
    def _create(self, fn_name, *args):
        """The ABI's create call ``fn_name(*args, &handle)``; the handle it returns becomes ``_h``."""
        h = C.c_void_p()
        _abi.check(getattr(self._lib, fn_name)(*args, C.byref(h)), fn_name)
        self._h = h

    def close(self):
        children, self._children = self._children, ()
        for ref in reversed(children):                      # most recently bound first
            child = ref()
            if child is not None:
                child.close()
        if self._open_children:
            # only when the cycle collector finalises a parent before its children: it clears the weak references to them before it
            # runs any finaliser.  The last child to close comes back here.
            self._close_pending = True
            return
        if getattr(self, "_h", None):
            getattr(self._lib, self._destroy)(self._h)
            self._h = None
        parent, self._parent = self._parent, None
        if parent is not None:
            parent._open_children -= 1
            if parent._close_pending:
                parent.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- torch plumbing ---------------------------------------------------------------------
    def _stream_ptr(self, stream):
        import torch
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        return C.c_void_p(stream.cuda_stream)

    def _torch_device(self):
        import torch
        return torch.device("cuda", self.device)

    def _check_tensor(self, t, shape, dtype, what=None):
        if not t.is_cuda or t.device.index != self.device:
            raise ValueError(f"{what or 'tensor'} must live on cuda:{self.device}")
        if tuple(t.shape) != tuple(shape) or t.dtype != dtype or not t.is_contiguous():
            raise ValueError((f"{what}: " if what else "") +
                             f"expected contiguous {dtype} tensor of shape {tuple(shape)}, got {t.dtype} {tuple(t.shape)}")

    def _check_vec(self, t, dtypes, what):
        """``[self.num_envs]`` of one of ``dtypes`` at any positive element stride.  Returns the stride."""
        if not t.is_cuda or t.device.index != self.device:
            raise ValueError(f"{what} must live on cuda:{self.device}")
        if t.dim() != 1 or t.shape[0] != self.num_envs or t.dtype not in dtypes:
            raise ValueError(f"{what}: expected a tensor of shape ({self.num_envs},) and dtype in {dtypes}, got {t.dtype} {tuple(t.shape)}")
        if self.num_envs > 1 and t.stride(0) < 1:
            raise ValueError(f"{what}: the element stride must be >= 1, got {t.stride(0)}")
        return max(int(t.stride(0)), 1)

    def _done_arg(self, done):
        """The done vector of ``include/quadgym.h`` -- uint8, bool or float32 ``[self.num_envs]`` at any positive stride, or None --
        as the ``(pointer, done_kind, done_stride)`` an entry point takes."""
        import torch
        if done is None:
            return None, _abi.DONE_U8, 1
        stride = self._check_vec(done, (torch.uint8, torch.bool, torch.float32), "done")
        return done.data_ptr(), (_abi.DONE_F32 if done.dtype == torch.float32 else _abi.DONE_U8), stride

    def _check_packed(self, t, what):
        """The plain env's packed rows: contiguous float32 ``[self.num_envs, self.obs_dim + 2]`` (obs, reward, done)."""
        import torch
        self._check_tensor(t, (self.num_envs, self.obs_dim + 2), torch.float32, what)

    ANY_ROWS = "n"          # `_check_rows(rows=ANY_ROWS)`: any number of rows >= 1 (spelled into the refusal's shape)

    def _check_rows(self, t, width, what, rows=None):
        """The one strided-rows check: float32 ``[rows, width]`` on this device (``rows`` defaults to ``self.num_envs``) whose rows are
        contiguous; the row stride is free (a column slice of a wider buffer).  A single column has no inner stride to violate and a
        single row no row stride.  Returns the row stride in floats, at least ``width``."""
        import torch
        rows = self.num_envs if rows is None else rows
        if not t.is_cuda or t.device.index != self.device:
            raise ValueError(f"{what} must live on cuda:{self.device}")
        if (t.dim() != 2 or t.shape[1] != width or t.dtype != torch.float32 or t.shape[0] < 1
                or (rows is not self.ANY_ROWS and t.shape[0] != rows)):
            raise ValueError(f"{what}: expected a float32 tensor of shape ({rows}, {width}), got {t.dtype} {tuple(t.shape)}")
        if (width > 1 and t.stride(1) != 1) or (t.shape[0] > 1 and t.stride(0) < width):
            raise ValueError(f"{what}: rows must be contiguous, at a row stride >= {width}; got strides {tuple(t.stride())}")
        return max(int(t.stride(0)), width)

    def _check_obs(self, t, n=None, what="obs"):
        """``_check_rows`` at the width ``self.obs_dim``, of ``n`` rows (None: any number >= 1).  Returns ``(rows, row stride)``."""
        stride = self._check_rows(t, self.obs_dim, what, self.ANY_ROWS if n is None else n)
        return int(t.shape[0]), stride
