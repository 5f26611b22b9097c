"""Handles bound to handles without a GPU (``Handle(parent=...)`` of quadruped_gym_amd/_handle.py): the C side's ``qg_po_destroy``
reads its walking layer and ``qg_walk_destroy`` reads and writes its simulator, so whatever the caller does -- close the simulator
first, drop the references in the wrong order -- the destroy functions must run in the order po, walk, sim, each once."""
import gc
import types

import pytest
import torch

from quadruped_gym_amd import _abi
from quadruped_gym_amd._handle import Handle
from quadruped_gym_amd.sim import BatchedSim
from quadruped_gym_amd.task_layers import ObsPack, WalkLayer

ORDER = ["qg_po_destroy", "qg_walk_destroy", "qg_destroy"]


class _RecordingLibrary:
    """Stands in for the loaded library: records the destroy calls, refuses every other one."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.endswith("destroy"):
            raise AssertionError(f"the library was called ({name})")
        return lambda h: self.calls.append((name, h)) or 0


def _bound(cls, token, parent=None):
    """An instance of a real handle class with ``token`` for a handle: the lifetime part only, nothing is created on a device."""
    h = cls.__new__(cls)
    Handle.__init__(h, 0, parent)
    h._h = token
    return h


def _chain(monkeypatch):
    """``(library, sim, walk, po)``; not a fixture, so that the test holds the only references."""
    lib = _RecordingLibrary()
    monkeypatch.setattr(_abi, "load_library", lambda: lib)
    sim = _bound(BatchedSim, "sim")
    walk = _bound(WalkLayer, "walk", sim)
    po = _bound(ObsPack, "po", walk)
    return lib, sim, walk, po


def test_closing_the_parent_closes_two_generations_of_children_first(monkeypatch):
    lib, sim, walk, po = _chain(monkeypatch)
    sim.close()
    assert lib.calls == [("qg_po_destroy", "po"), ("qg_walk_destroy", "walk"), ("qg_destroy", "sim")]
    assert sim._h is None and walk._h is None and po._h is None


def test_children_close_most_recently_bound_first(monkeypatch):
    lib, sim, walk, po = _chain(monkeypatch)
    later = _bound(WalkLayer, "later", sim)
    sim.close()
    assert [h for _, h in lib.calls] == ["later", "po", "walk", "sim"]
    assert later._h is None


@pytest.mark.parametrize("first", ["sim", "walk", "po"])
def test_a_second_close_calls_nothing(monkeypatch, first):
    lib, sim, walk, po = _chain(monkeypatch)
    handles = {"sim": sim, "walk": walk, "po": po}
    handles[first].close()
    sim.close()
    assert [name for name, _ in lib.calls] == ORDER
    seen = list(lib.calls)
    for h in (sim, walk, po, po, walk, sim):
        h.close()
    assert lib.calls == seen


def test_binding_to_a_closed_parent_raises(monkeypatch):
    lib, sim, walk, po = _chain(monkeypatch)
    walk.close()
    with pytest.raises(ValueError, match="closed"):
        _bound(ObsPack, "late", walk)
    sim.close()
    with pytest.raises(ValueError, match="closed"):
        _bound(WalkLayer, "late", sim)
    assert [h for _, h in lib.calls] == ["po", "walk", "sim"]


def test_dropping_the_references_parent_first_still_destroys_children_first(monkeypatch):
    lib, sim, walk, po = _chain(monkeypatch)
    del sim
    gc.collect()
    assert lib.calls == []              # the walking layer holds its simulator
    del walk
    gc.collect()
    assert lib.calls == []              # the pack holds its walking layer
    del po
    gc.collect()
    assert [name for name, _ in lib.calls] == ORDER


@pytest.mark.parametrize("held", ["all", "sim", "walk", "po"])
def test_a_chain_collected_as_part_of_a_reference_cycle_keeps_the_order(monkeypatch, held):
    """An env that a cycle reaches (``trainer.env = env; env.callback = trainer.method``) is freed by the cycle collector, which clears
    the weak references to the children before it runs any finaliser, the simulator's possibly first."""
    lib, sim, walk, po = _chain(monkeypatch)
    gc.collect()
    owner = types.SimpleNamespace()
    owner.me = owner
    owner.held = {"all": (sim, walk, po), "sim": sim, "walk": (walk, sim), "po": (sim, po)}[held]
    sim.back = walk.back = po.back = owner              # every handle is on the cycle itself, whatever the owner holds
    del sim, walk, po, owner
    assert held != "all" or lib.calls == []             # what the owner does not hold is freed by its reference count, pack first
    gc.collect()
    assert lib.calls == [("qg_po_destroy", "po"), ("qg_walk_destroy", "walk"), ("qg_destroy", "sim")]


def test_a_child_whose_create_failed_does_not_keep_its_parent_open(monkeypatch):
    lib, sim, walk, po = _chain(monkeypatch)
    failed = _bound(ObsPack, None, walk)               # bound, but its create call returned no handle
    del failed
    sim.close()
    assert [h for _, h in lib.calls] == ["po", "walk", "sim"]


def test_step_device_checks_its_tensors_before_any_library_call(monkeypatch):
    """The recording library refuses everything but a destroy; the stand-ins claim to be on the device (there is none here)."""
    lib, sim, walk, po = _chain(monkeypatch)
    walk.num_envs = po.num_envs = 3
    po.obs_dim = 52

    def fake(shape, dtype=torch.float32, contiguous=True):
        return types.SimpleNamespace(is_cuda=True, device=types.SimpleNamespace(index=0), shape=shape, dtype=dtype,
                                     is_contiguous=lambda: contiguous, data_ptr=lambda: 0)
    for layer in (walk, po):
        D = layer.obs_dim
        good = dict(actions=fake((3, 12)), obs=fake((3, D)), reward=fake((3,)), done=fake((3,), torch.uint8), components=fake((3, 11)))
        bad = [dict(actions=torch.zeros((3, 12))), dict(obs=fake((3, D), torch.float64)), dict(obs=fake((4, D))),
               dict(obs=fake((3, D), contiguous=False)), dict(reward=fake((3, 1))), dict(done=fake((3,), torch.int32)),
               dict(components=fake((3, 10)))] + ([dict(terminal_obs=fake((3, D - 1)))] if layer is po else [])
        for swap in bad:
            with pytest.raises(ValueError, match=next(iter(swap))):
                layer.step_device(**dict(good, **swap))
        with pytest.raises(AssertionError, match="step_device"):         # a good set of tensors does reach the library
            layer.step_device(**dict(good, done=fake((3,), torch.bool)), stream=types.SimpleNamespace(cuda_stream=0))
