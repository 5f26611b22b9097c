"""Shared helpers for the test-suite (state sampling, model variants, one oracle model per env, body wrenches, hipGraph capture)."""
import contextlib
import ctypes as C
import json
import lzma
import os
import re
import shutil

import numpy as np
import pytest

NQ, NV, NU, NBODY = 19, 18, 12, 13
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def header_text():
    return open(os.path.join(ROOT, "include", "quadgym.h")).read()


def header_define(header, name):
    """The integer a `#define name ...` of the header stands for: a literal, or another macro's name (an alias), followed."""
    value = re.search(r"#define %s (\w+)" % name, header).group(1)
    return int(value) if value.isdigit() else header_define(header, value)


@contextlib.contextmanager
def capture_graph(graph, device="cuda:0"):
    """Captures the body into ``graph`` and leaves no stream behind: which hardware queue the streams that LATER tests of this process
    create land on depends on the streams alive, wherever the capturing module is collected.  So the capture stream is
    created through the HIP runtime and destroyed again (``torch.cuda.Stream()`` takes one from torch's pool for good), and the capture
    is begun and ended by hand (the first ``torch.cuda.graph(...)`` of a process takes a pool stream of its own, whether it is given one
    or not)."""
    import torch
    from quadruped_gym_amd import _abi
    lib, handle = _abi.load_library(), C.c_void_p()          # (the runtime is a dependency of the library: one lookup serves both)
    assert lib.hipStreamCreateWithFlags(C.byref(handle), C.c_uint(1)) == 0       # hipStreamNonBlocking
    try:
        torch.cuda.synchronize()
        with torch.cuda.stream(torch.cuda.ExternalStream(handle.value, device=device)):
            graph.capture_begin()
            try:
                yield
            finally:
                graph.capture_end()
    finally:
        torch.cuda.synchronize()
        assert lib.hipStreamDestroy(handle) == 0


def reference_model(tmp_dir):
    """The reference robot's MJCF scene, unpacked from tests/golden/quadruped_model (tools/make_model_fixture.py) into
    `tmp_dir`: the two XML files and every mesh's vertex positions.  Returns the path of scene.xml."""
    src = os.path.join(GOLDEN, "quadruped_model")
    out = os.path.join(str(tmp_dir), "quadruped")
    os.makedirs(os.path.join(out, "mesh"), exist_ok=True)
    for name in ("scene.xml", "quadruped.xml"):
        shutil.copyfile(os.path.join(src, name), os.path.join(out, name))
    for name in os.listdir(os.path.join(src, "mesh")):
        with lzma.open(os.path.join(src, "mesh", name)) as fh, open(os.path.join(out, "mesh", name[:-len(".xz")]), "wb") as dst:
            dst.write(fh.read())
    return os.path.join(out, "scene.xml")


def random_state(rng, model, z=1.0, vel=1.0, joint_margin=0.05):
    """A random state well inside the joint ranges, base at height z."""
    qpos = np.zeros(NQ)
    qpos[0:2] = rng.uniform(-0.5, 0.5, 2)
    qpos[2] = z
    q = rng.normal(size=4)
    qpos[3:7] = q / np.linalg.norm(q)
    for j in range(12):
        lo, hi = model.jnt_range[j][0], model.jnt_range[j][1]
        qpos[7 + j] = rng.uniform(lo + joint_margin, hi - joint_margin)
    qvel = vel * rng.normal(size=NV)
    qvel[6:] *= 3.0
    return qpos, qvel


def make_conservative(model):
    """Strip every dissipative / driven term: what is left is a free-floating tree under gravity."""
    model.free_damping = 0.0
    for j in range(12):
        model.jnt_damping[j] = 0.0
        model.act_kp[j] = 0.0
        model.act_kv[j] = 0.0
        model.jnt_range[j][0] = -100.0
        model.jnt_range[j][1] = 100.0
    return model


# ---- the table robot: servo gains +10 %, contact stiffness -10 % (any robot but the compiled-in one runs the table-driven kernels) ----
def write_table_robot(directory):
    """The table robot as a model JSON in `directory`: its path."""
    d = json.load(open(os.path.join(ROOT, "quadruped-gym_amd", "model", "quadruped_model.json")))
    for act in d["actuators"]:
        act["kp"] *= 1.1
    d["contact"]["stiffness"] *= 0.9
    path = os.path.join(str(directory), "tweaked.json")
    with open(path, "w") as fh:
        json.dump(d, fh)
    return path


def table_model(model, stiffness=0.9):
    """The same tweak of a qg_model in memory (`stiffness=1.0`: the servo gains alone)."""
    for j in range(12):
        model.act_kp[j] *= 1.1
    model.contact_stiffness *= stiffness
    return model


@pytest.fixture(scope="module")
def table_robot(tmp_path_factory):
    """(path of the table robot's JSON, its qg_model)."""
    from quadruped_gym_amd.model.loader import load_model
    path = write_table_robot(tmp_path_factory.mktemp("robot"))
    return path, load_model(path)[0]


# ---- one model per env ----------------------------------------------------------------------------------------------------------------
def env_model(oracle, base, row):
    """The qg_model one env runs with `row` (f32 values, the table of include/quadgym.h), in f64: the payload combined with the FRAME
    by the parallel-axis rule, the FRAME's inertia expressed about the new centre of mass."""
    m = oracle.default_model()
    C.memmove(C.byref(m), C.byref(base), C.sizeof(m))
    row = np.asarray(row, np.float64)
    m.contact_friction = row[0]
    dm, p = row[1], row[2:5]
    m0, c0 = base.body_mass[0], np.array(base.body_ipos[0][:])
    I = base.body_inertia[0]
    I0 = np.array([[I[0], I[3], I[4]], [I[3], I[1], I[5]], [I[4], I[5], I[2]]])
    m1 = m0 + dm
    c1 = (m0 * c0 + dm * p) / m1

    def shift(mass, d):
        return mass * (np.dot(d, d) * np.eye(3) - np.outer(d, d))
    I1 = I0 + shift(m0, c0 - c1) + shift(dm, p - c1)
    m.body_mass[0] = m1
    for i in range(3):
        m.body_ipos[0][i] = c1[i]
    for i, v in enumerate([I1[0, 0], I1[1, 1], I1[2, 2], I1[0, 1], I1[0, 2], I1[1, 2]]):
        m.body_inertia[0][i] = v
    for j in range(12):
        m.act_kp[j] = base.act_kp[j] * row[5]
        m.act_kv[j] = base.act_kv[j] * row[6]
        m.act_forcerange[j][0] = base.act_forcerange[j][0] * row[7]
        m.act_forcerange[j][1] = base.act_forcerange[j][1] * row[7]
        m.jnt_damping[j] = base.jnt_damping[j] * row[8]
    m.contact_stiffness = base.contact_stiffness * row[9]
    m.contact_damping = base.contact_damping * row[10]
    return m


def oracle_step_each(oracle, models, task, state, actions):
    """One oracle env-step of state i on models[i] with actions[i].  Returns a dict of per-env arrays -- ``obs``, ``reward``, ``done``,
    ``comps`` and the post-step ``qpos`` / ``qvel`` / ``act`` / ``nstep`` -- and ``batches``, the one-env oracle batches after the
    step."""
    qpos, qvel, act, nstep = state
    actions = np.asarray(actions, np.float64)
    rows, batches = [], []
    for i, model in enumerate(models):
        b = oracle.Batch(model, task, 1)
        b.set_state(np.asarray(qpos[i:i + 1], np.float64), np.asarray(qvel[i:i + 1], np.float64), np.asarray(act[i:i + 1], np.float64),
                    None, nstep[i:i + 1])
        obs, rew, done, comps = b.step(actions[i:i + 1])
        q, v, a, _, ns = b.get_state()
        rows.append((obs[0], rew[0], done[0], comps[0], q[0], v[0], a[0], ns[0]))
        batches.append(b)
    out = dict(zip(("obs", "reward", "done", "comps", "qpos", "qvel", "act", "nstep"), (np.array(x) for x in zip(*rows))))
    out["batches"] = batches
    return out


def oracle_per_env(oracle, base, task, rows, state, actions):
    """One env-step of every env on its own model (`base` with the env's dynamics row); returns (obs, reward, comps, qpos, qvel, act)
    stacked."""
    out = oracle_step_each(oracle, [env_model(oracle, base, row) for row in rows], task, state, actions)
    return [out[k] for k in ("obs", "reward", "comps", "qpos", "qvel", "act")]


# ---- body wrenches as a generalized force -----------------------------------------------------------------------------------------------
def _leg_bodies(j):
    """Bodies hinge j moves: its child body j + 1 and the links below it on the same leg."""
    leg = j // 3
    return range(j + 1, 3 * leg + 4)


def generalized_force(oracle, model, qpos, F, T):
    """tau [18] of world-frame forces F [13, 3] (at each body's centre of mass) and torques T [13, 3] (pinned without a GPU by
    tests/test_external_wrench_checker.py)."""
    xpos, xmat, xcom = oracle.kinematics(model, qpos)
    F, T = np.asarray(F, np.float64), np.asarray(T, np.float64)
    tau = np.zeros(NV)
    p0, R0 = xpos[0], xmat[0]
    for b in range(NBODY):
        tau[0:3] += F[b]
        tau[3:6] += R0.T @ (T[b] + np.cross(xcom[b] - p0, F[b]))
    for j in range(12):
        axis = xmat[j + 1] @ np.array(model.jnt_axis[j][:])
        anchor = xpos[j + 1]
        for b in _leg_bodies(j):
            tau[6 + j] += axis @ (T[b] + np.cross(xcom[b] - anchor, F[b]))
    return tau


def rotz(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])


def quat_mul(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw])
