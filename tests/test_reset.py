"""reset_data / reset_data_keyframe: per-world masks and keyframes, on the host (CPU device) and in one launch of csrc/reset.hpp on the GPU,
and the auto-resetting StepGraph.  The truth is tests/reset_truth.py; a reset only copies and fills, so every comparison is bitwise.

The GPU tests share one model (reset_model) built to reach every branch of k_reset: a free and a ball joint (nq != nv), a filter actuator
(na > 0), 14 bodies (6 nbody = 84 > 64: the lane loop over xfrc_applied runs twice), two mocap bodies whose mocap ids run against their body order,
a joint equality, a delayed actuator (nsample 3) and two sensors with buffers (nsample 5 and, three values wide, nsample 2), three keyframes
with mpos, mquat, act, ctrl and a time, and per-world qpos0, body_pos and timestep.
"""

import numpy as np
import pytest

import reset_truth as rt
import mujoco_warp_amd as mjw
from mujoco_warp_amd import _abi, io, mjcf
from mujoco_warp_amd.device import DeviceArray

NQ, NV, NA, NU, NMOCAP = 20, 18, 1, 3, 2


def _keyframes():
  rng = np.random.default_rng(11)
  unit = lambda: (lambda q: q / np.linalg.norm(q))(rng.normal(size=4))
  fmt = lambda a: " ".join(f"{x:.6f}" for x in np.ravel(a))
  out = []
  for i, time in enumerate((0.37, 1.5, 0.004)):
    qpos = np.concatenate([[0.1 * i, -0.2, 0.3 + 0.1 * i], unit(), unit(), rng.uniform(-0.3, 0.3, 7), rng.uniform(-0.05, 0.05, 2)])
    out.append(f'<key name="k{i}" time="{time}" qpos="{fmt(qpos)}" qvel="{fmt(rng.uniform(-0.2, 0.2, NV))}" act="{fmt(rng.uniform(-1, 1, NA))}" '
               f'ctrl="{fmt(rng.uniform(-0.5, 0.5, NU))}" mpos="{fmt(rng.uniform(-1, 1, 3 * NMOCAP))}" mquat="{fmt([unit(), unit()])}"/>')
  return "".join(out)


def _chain(n, k=1):
  if k > n:
    return ""
  tip = '<site name="tip" pos="0 0 -.12"/>' if k == n else ""
  return (f'<body name="l{k}" pos="0 0 -.12"><joint name="h{k}" type="hinge" axis="0 1 0" damping=".05"/><geom type="capsule" fromto="0 0 0 0 0 -.12" size=".02"/>'
          f'{tip}{_chain(n, k + 1)}</body>')


RESET_XML = f"""
<mujoco><option timestep="0.002"/>
<default><geom contype="0" conaffinity="0"/></default>
<worldbody>
  <geom name="floor" type="plane" size="0 0 .05" contype="1" conaffinity="1"/>
  <body name="m0" mocap="true" pos="-1 0 .5"><geom type="box" size=".05 .05 .05"/></body>
  <body name="free" pos="0 0 .09"><freejoint/><geom type="sphere" size=".1" contype="1" conaffinity="1"/></body>
  <body name="arm" pos="1 0 1.5"><joint name="ball" type="ball" damping=".02"/><geom type="capsule" fromto="0 0 0 0 0 -.12" size=".02"/>{_chain(7)}</body>
  <body name="p1" pos="0 1 .5"><joint name="s1" type="slide" axis="1 0 0" damping="1"/><geom type="sphere" size=".05"/></body>
  <body name="p2" pos="0 1.5 .5"><joint name="s2" type="slide" axis="1 0 0" damping="1"/><geom type="sphere" size=".05"/></body>
  <body name="m1" mocap="true" pos="-1 1 .5" quat="0.8 0 0.6 0"><geom type="box" size=".05 .05 .05"/></body>
</worldbody>
<equality><joint joint1="s1" joint2="s2" polycoef="0 1 0 0 0"/></equality>
<actuator>
  <general name="filt" joint="h1" dyntype="filter" dynprm="0.05" gainprm="2"/>
  <motor name="late" joint="h2" delay="0.006" nsample="3"/>
  <motor name="push" joint="s1"/>
</actuator>
<sensor>
  <jointvel joint="h1"/>
  <jointpos joint="h3" delay="0.004" nsample="5" interp="linear"/>
  <framepos objtype="site" objname="tip" nsample="2"/>
</sensor>
<keyframe>{_keyframes()}</keyframe>
</mujoco>
"""


def reset_host_model():
  mjm = mjcf.from_xml_string(RESET_XML)
  assert (mjm.nq, mjm.nv, mjm.na, mjm.nu, mjm.nmocap, mjm.nkey, mjm.neq) == (NQ, NV, NA, NU, NMOCAP, 3, 1) and mjm.nbody == 14 and mjm.nhistory > 0
  # mocap ids against the body order: body m0 (the first body) gets mocap id 1, m1 (the last) id 0; the keyframes' mpos / mquat are per mocap id
  mjm.body_mocapid = np.where(mjm.body_mocapid >= 0, 1 - mjm.body_mocapid, -1).astype(np.int32)
  assert rt.mocap_bodies(mjm) == [13, 1]
  return mjm


def reset_model(nworld):
  """(host model, Model with per-world qpos0 / body_pos / timestep, the batched host values for the truth)"""
  mjm = reset_host_model()
  m = mjw.put_model(mjm, batch_sizes={"qpos0": nworld, "body_pos": nworld, "timestep": nworld})
  rng = np.random.default_rng(nworld)
  batched = dict(qpos0=m.qpos0.numpy() + rng.uniform(-0.01, 0.01, (nworld, NQ)).astype(np.float32),
                 body_pos=m.body_pos.numpy() + rng.uniform(-0.01, 0.01, (nworld, 14, 3)).astype(np.float32),
                 timestep=(0.002 + 0.0001 * (np.arange(nworld) % 3)).astype(np.float32))
  m.qpos0.assign(batched["qpos0"])
  m.body_pos.assign(batched["body_pos"])
  m.opt.timestep.assign(batched["timestep"])
  return mjm, m, batched


def snapshot(d):
  """Every declared array of Data (contact_ / efc_ included) as numpy copies."""
  out = {}
  for name in io._DATA_ARRAYS:
    a = io._get_data_field(d, name)
    if a is not None:
      out[name] = a.numpy().copy()
  return out


def assert_same(got, want, what=""):
  assert got.keys() == want.keys()
  for name in want:
    np.testing.assert_array_equal(got[name], want[name], err_msg=f"{what}: Data.{name}")


def scramble(d, seed):
  """User-written inputs a reset has to restore, set to junk."""
  rng = np.random.default_rng(seed)
  for name in ("qfrc_applied", "xfrc_applied", "mocap_pos", "mocap_quat", "qacc_warmstart"):
    a = getattr(d, name)
    a.assign(rng.uniform(-1, 1, a.shape).astype(np.float32))
  d.eq_active.assign(rng.integers(0, 2, d.eq_active.shape).astype(np.int32))


def mixed_mask(nworld):
  mask = (np.arange(nworld) % 3 != 1)
  mask[-1] = True
  return mask


def mixed_keys(nworld, nkey=3):
  keys = (np.arange(nworld) * 2 + 1) % nkey
  if nworld >= 4:  # two worlds that the mask selects carry a key outside [0, nkey): they are not reset
    keys[0], keys[3] = -1, nkey + 4
  return keys.astype(np.int32)


def restore(d, snap):
  import torch

  for name, v in snap.items():
    t = io._get_data_field(d, name).t
    if t.numel():
      t.copy_(torch.from_numpy(v.view(np.int32) if v.dtype == np.uint32 else v))


# --------------------------------------------------------------------------------------------------------- with or without a GPU
# (no kernel is needed to set these up: without a GPU the calls below take the numpy path of io.py, with one the launch of csrc/reset.hpp --
# the same truth holds for both)
def _host_data(mjm, nworld):
  m = mjw.put_model(mjm)
  d = mjw.make_data(mjm, nworld=nworld)
  rng = np.random.default_rng(3)
  for name in ("qpos", "qvel", "act", "ctrl", "qacc", "time"):  # (no kernels on the CPU device: a state that a step could have left)
    a = getattr(d, name)
    a.assign(rng.uniform(-1, 1, a.shape).astype(np.float32))
  for name in rt.COUNTERS + ("nacon", "ws_conadr"):
    a = getattr(d, name)
    a.assign(rng.integers(1, 9, a.shape).astype(np.int32))
  d.history.assign(rng.uniform(-1, 1, d.history.shape).astype(np.float32))
  scramble(d, 4)
  return m, d


@pytest.mark.parametrize("with_mask", [False, True])
def test_keyframe_per_world(with_mask):
  """key = [1, -1, 0, 7, 1] on 5 worlds, nkey 3: worlds 0, 2 and 4 take their keyframe, worlds 1 and 3 are untouched; with a mask on top, only the
  worlds both select."""
  mjm = reset_host_model()
  m, d = _host_data(mjm, 5)
  before = snapshot(d)
  keys = [1, -1, 0, 7, 1]
  mask = np.array([True, True, False, True, True]) if with_mask else None
  mjw.reset_data_keyframe(m, d, keys, reset=mask)
  after = snapshot(d)
  assert_same(after, rt.expected(mjm, before, mask=mask, keys=keys))
  reset_worlds = [0, 4] if with_mask else [0, 2, 4]
  for w in range(5):
    if w in reset_worlds:
      np.testing.assert_array_equal(after["qpos"][w], mjm.key_qpos[keys[w]].astype(np.float32))
      assert after["time"][w] == np.float32(mjm.key_time[keys[w]]) and after["nefc"][w] == 0
      np.testing.assert_array_equal(after["mocap_pos"][w].ravel(), mjm.key_mpos[keys[w]].astype(np.float32))
    else:
      for name in before:
        if before[name].shape[:1] == (5,):
          np.testing.assert_array_equal(after[name][w], before[name][w], err_msg=name)
  np.testing.assert_array_equal(after["nacon"], before["nacon"])  # the per-world form leaves the global counters alone


def test_masked_reset_and_int_key_match_the_truth():
  mjm = reset_host_model()
  for kw, call in ((dict(), lambda m, d, r: mjw.reset_data(m, d, r)), (dict(key=2), lambda m, d, r: mjw.reset_data_keyframe(m, d, 2, r))):
    for mask in (None, np.array([1, 0, 0, 1, 1], dtype=np.int64), DeviceArray.from_numpy(np.array([False, True, True, False, True]))):
      m, d = _host_data(mjm, 5)
      before = snapshot(d)
      call(m, d, mask)
      hm = None if mask is None else np.asarray(mask.numpy() if isinstance(mask, DeviceArray) else mask) != 0
      assert_same(snapshot(d), rt.expected(mjm, before, mask=hm, **kw), f"{kw} {mask}")


def test_argument_checks():
  """A mask of the wrong shape or of float dtype, a key array of the wrong shape or of float dtype, an int key out of range: ValueError, and
  nothing is written."""
  import torch

  mjm = reset_host_model()
  m = mjw.put_model(mjm)
  d = mjw.make_data(mjm, nworld=5)
  d.qvel.fill_(0.25)
  ok_keys = np.zeros(5, dtype=np.int32)
  for bad_mask in (np.ones(4, dtype=bool), np.ones((5, 1), dtype=bool), np.ones(5, dtype=np.float32), torch.ones(5), DeviceArray.zeros((6,), dtype=np.int32)):
    with pytest.raises(ValueError, match="reset must"):
      mjw.reset_data(m, d, bad_mask)
    with pytest.raises(ValueError, match="reset must"):
      mjw.reset_data_keyframe(m, d, ok_keys, bad_mask)
  for bad_key in (np.zeros(4, dtype=np.int32), np.zeros((1, 5), dtype=np.int32), np.zeros(5, dtype=np.float32), [0.0, 1.0, 2.0, 0.0, 1.0],
                  np.zeros(5, dtype=bool), torch.zeros(5, dtype=torch.float64)):
    with pytest.raises(ValueError, match="key must"):
      mjw.reset_data_keyframe(m, d, bad_key)
  for bad_int in (-1, 3):
    with pytest.raises(ValueError, match="out of range"):
      mjw.reset_data_keyframe(m, d, bad_int)
  assert (d.qvel.numpy() == 0.25).all()


def test_abi_lists_the_unit_and_the_entry_points():
  assert _abi.DEFINES["MJH_ABI_VERSION"] == 45
  assert "reset_tu.hip" in _abi.UNITS and "reset.hpp" in _abi.HEADERS and "reset_tu.hip" not in _abi.UNIT_FLAGS
  assert {"mjh_reset", "mjh_graph_create_reset", "mjh_graph_create"} <= set(_abi.FUNCTIONS)
  names = [n for n, _, _ in _abi.RESET_FIELDS]
  assert names[:6] == ["mask_u8", "mask_i32", "keys", "key", "nkey", "nkey_mocap"] and names[-1] == "mocap_bodyid"
  # MjhModel and MjhData did not grow: what the kernel needs beyond them travels in MjhReset
  assert not any("key_" in n for n, _, _ in _abi.MODEL_FIELDS) and [n for n, _, _ in _abi.DATA_FIELDS][-1] == "ws_contact"


def test_device_tables_follow_a_rebinding():
  """The device copies of the keyframe tables and eq_active0 are made at put_model and rebuilt when one of the attributes is re-bound (an in-place
  edit is not seen: documented)."""
  mjm = reset_host_model()
  m = mjw.put_model(mjm)
  tabs = io._reset_tables(m)
  np.testing.assert_array_equal(tabs["key_qpos"].numpy(), mjm.key_qpos.astype(np.float32))
  np.testing.assert_array_equal(tabs["key_mquat"].numpy(), mjm.key_mquat.astype(np.float32))
  assert tabs["mocap_bodyid"].numpy().tolist() == [13, 1] and tabs["eq_active0"].numpy().tolist() == [1]
  io.c_model(m)
  assert io._reset_tables(m) is tabs  # nothing re-bound: the same device arrays
  m.key_qvel = m.key_qvel + 1.0
  assert m._dirty
  io.c_model(m)
  new = m._reset_dev[1]
  assert new is not tabs and new["mocap_bodyid"] is tabs["mocap_bodyid"]
  np.testing.assert_array_equal(new["key_qvel"].numpy(), mjm.key_qvel.astype(np.float32) + 1.0)


# ------------------------------------------------------------------------------------------------------------------------ on the GPU
def _stepped(nworld, nstep=6):
  mjm, m, batched = reset_model(nworld)
  d = mjw.make_data(m, nworld=nworld)
  d.qpos.assign(batched["qpos0"])
  rng = np.random.default_rng(100 + nworld)
  d.ctrl.assign(rng.uniform(-0.5, 0.5, d.ctrl.shape).astype(np.float32))
  d.qvel.assign(rng.uniform(-0.1, 0.1, d.qvel.shape).astype(np.float32))
  for _ in range(nstep):
    mjw.step(m, d)
  scramble(d, nworld)
  return mjm, m, batched, d


FORMS = ("reset_data", "int_key", "array_key", "no_mask", "no_mask_int_key")


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("nworld", [1, 5, 67])
def test_field_sweep(nworld, form):
  """Step 6 times, snapshot, reset: the selected worlds equal the truth; every other world and every field a reset does not write -- every
  declared array of Data is compared -- is bit-identical to the snapshot."""
  mjm, m, batched, d = _stepped(nworld)
  before = snapshot(d)
  assert before["time"].min() > 0 and before["nefc"].min() > 0 and before["ws_ncon"].max() > 0 and np.abs(before["history"]).max() > 0 and np.abs(before["act"]).max() > 0
  mask = mixed_mask(nworld)
  dmask = DeviceArray.from_numpy(mask)
  if form == "reset_data":
    mjw.reset_data(m, d, dmask)
    want = rt.expected(mjm, before, mask=mask, batched=batched)
  elif form == "int_key":
    mjw.reset_data_keyframe(m, d, 1, dmask)
    want = rt.expected(mjm, before, mask=mask, key=1, batched=batched)
  elif form == "array_key":
    keys = mixed_keys(nworld)
    mjw.reset_data_keyframe(m, d, DeviceArray.from_numpy(keys), dmask)
    want = rt.expected(mjm, before, mask=mask, keys=keys, batched=batched)
    if nworld >= 4:
      assert mask[0] and mask[3]
      np.testing.assert_array_equal(want["qpos"][[0, 3]], before["qpos"][[0, 3]])
  elif form == "no_mask":
    mjw.reset_data(m, d)
    want = rt.expected(mjm, before, batched=batched)
  else:
    mjw.reset_data_keyframe(m, d, 2)
    want = rt.expected(mjm, before, key=2, batched=batched)
  after = snapshot(d)
  assert_same(after, want, form)
  written = set(rt.WRITTEN)
  for name in before:  # (the truth said so already; stated once more for what a stray write would hit)
    if name not in written:
      np.testing.assert_array_equal(after[name], before[name], err_msg=f"stray write: Data.{name}")


SLEEP_XML = """
<mujoco><option timestep="0.004"><flag sleep="enable"/></option>
<worldbody><geom type="plane" size="0 0 .05"/>
  <body pos="0 0 .0999"><freejoint/><geom type="box" size=".1 .1 .1"/></body>
  <body pos="1 0 .0999"><freejoint/><geom type="box" size=".1 .1 .1"/></body>
</worldbody></mujoco>
"""


@pytest.mark.gpu
def test_sleeping_worlds_wake_on_reset():
  mjm = mjcf.from_xml_string(SLEEP_XML)
  m = mjw.put_model(mjm)
  assert m.sleep_enabled
  d = mjw.make_data(mjm, nworld=4)
  fresh = snapshot(mjw.make_data(mjm, nworld=4))
  for _ in range(100):
    mjw.step(m, d)
  before = snapshot(d)
  assert (before["tree_asleep"] != fresh["tree_asleep"]).any(axis=1).all()  # the counters ran (or the trees sleep) in every world
  mask = np.array([True, False, True, False])
  mjw.reset_data(m, d, DeviceArray.from_numpy(mask))
  after = snapshot(d)
  for name in rt.SLEEP_TABLES:
    np.testing.assert_array_equal(after[name][mask], fresh[name][mask], err_msg=name)
    np.testing.assert_array_equal(after[name][~mask], before[name][~mask], err_msg=name)
  assert_same(after, rt.expected(mjm, before, mask=mask))


@pytest.mark.gpu
def test_no_host_trip(monkeypatch):
  """With a device mask and device keys a reset reads nothing back and uploads nothing: DeviceArray.numpy / assign are never called."""
  import torch

  mjm, m, batched, d = _stepped(5)
  before = snapshot(d)
  mask, keys = mixed_mask(5), mixed_keys(5)
  dmask, dkeys = DeviceArray.from_numpy(mask), DeviceArray.from_numpy(keys)
  sig = int(mjw.State.QPOS) | int(mjw.State.QVEL)
  state = DeviceArray.zeros((5, io.state_size(m, sig)))
  state.fill_(0.5)

  def refuse(*a, **k):
    raise AssertionError("host trip")

  with monkeypatch.context() as mp:
    mp.setattr(DeviceArray, "numpy", refuse)
    mp.setattr(DeviceArray, "assign", refuse)
    mjw.reset_data(m, d, dmask)
    mjw.reset_data_keyframe(m, d, dkeys, dmask)
    mjw.reset_data_keyframe(m, d, dkeys.t.to(torch.int64), dmask.t)
    io.set_state(m, d, state, sig, active=dmask)
    io.get_state(m, d, state, sig, active=dmask.t)
  want = rt.expected(mjm, rt.expected(mjm, before, mask=mask, batched=batched), mask=mask, keys=keys, batched=batched)
  want["qpos"][mask], want["qvel"][mask] = 0.5, 0.5
  assert_same(snapshot(d), want)
  assert (state.numpy() == 0.5).all()


@pytest.mark.gpu
def test_mask_dtypes_agree():
  import torch

  mjm, m, batched, d0 = _stepped(5)
  mask = mixed_mask(5)
  masks = dict(bool_da=DeviceArray.from_numpy(mask), int32_da=DeviceArray.from_numpy(mask.astype(np.int32) * 7), torch_bool=torch.from_numpy(mask).to(d0.qpos.t.device),
               numpy_bool=mask, torch_int64=torch.from_numpy(mask.astype(np.int64) * -3).to(d0.qpos.t.device))
  start = snapshot(d0)
  results = {}
  for name, dm in masks.items():
    restore(d0, start)
    mjw.reset_data_keyframe(m, d0, 0, dm)
    results[name] = snapshot(d0)
  want = rt.expected(mjm, start, mask=mask, key=0, batched=batched)
  for name, got in results.items():
    assert_same(got, want, name)


CONTACT_XML = """
<mujoco><option timestep="0.003"/>
<worldbody><geom type="plane" size="0 0 .05"/>
  <body name="a" pos="0 0 .099"><freejoint/><geom type="sphere" size=".1"/><site name="sa"/></body>
  <body name="b" pos=".03 .01 .28"><freejoint/><geom type="sphere" size=".09"/></body>
  <body name="c" pos=".5 0 .059" euler="90 0 0"><freejoint/><geom type="capsule" size=".06 .15"/></body>
</worldbody>
<sensor><framepos objtype="body" objname="b"/><framelinvel objtype="body" objname="c"/><accelerometer site="sa"/><touch site="sa"/></sensor>
</mujoco>
"""


@pytest.mark.gpu
def test_reset_worlds_step_like_fresh_ones():
  """Step 6, reset worlds {0, 2} of 5, step 6 more: the reset worlds are where a fresh Data is after 6 steps (the engine is deterministic and its
  results do not depend on what earlier steps left in Data)."""
  mjm = mjcf.from_xml_string(CONTACT_XML)
  m = mjw.put_model(mjm)
  d, fresh = mjw.make_data(mjm, nworld=5), mjw.make_data(mjm, nworld=5)
  rng = np.random.default_rng(5)
  d.qvel.assign(rng.uniform(-0.5, 0.5, d.qvel.shape).astype(np.float32))  # (the worlds differ before the reset)
  for _ in range(6):
    mjw.step(m, d)
  mjw.reset_data(m, d, DeviceArray.from_numpy(np.array([1, 0, 1, 0, 0], dtype=np.int32)))
  for _ in range(6):
    mjw.step(m, d)
    mjw.step(m, fresh)
  assert fresh.ws_ncon.numpy().min() > 0
  for name in ("qpos", "qvel", "sensordata"):
    np.testing.assert_array_equal(getattr(d, name).numpy()[[0, 2]], getattr(fresh, name).numpy()[[0, 2]], err_msg=name)
  assert (d.qpos.numpy()[1] != fresh.qpos.numpy()[1]).any()


@pytest.mark.gpu
@pytest.mark.parametrize("with_keys", [False, True])
def test_graph_resets_then_steps(with_keys):
  """StepGraph(m, d, reset=mask[, key=keys]): 8 launches with the mask (and the keys) rewritten on the device in between are bit-identical to the
  eager reset + step; StepGraph(m, d) replays the plain step as before."""
  import torch

  W = 5
  mjm, m, batched, dg = _stepped(W, nstep=2)
  de = mjw.make_data(m, nworld=W)
  restore(de, snapshot(dg))
  rng = np.random.default_rng(8)
  dev = dg.qpos.t.device
  masks = torch.from_numpy(rng.integers(0, 2, (8, W)).astype(np.int32)).to(dev)
  keyseq = torch.from_numpy(rng.integers(-1, 4, (8, W)).astype(np.int32)).to(dev)
  mask, keys = DeviceArray.zeros((W,), dtype=np.int32), DeviceArray.zeros((W,), dtype=np.int32)
  g = mjw.StepGraph(m, dg, reset=mask, key=keys if with_keys else None)
  for name in ("qpos", "qvel", "act", "ctrl", "time", "history", "qacc_warmstart"):  # constructing the graph does not advance the simulation
    np.testing.assert_array_equal(getattr(dg, name).numpy(), getattr(de, name).numpy(), err_msg=name)
  for i in range(8):
    mask.t.copy_(masks[i])
    keys.t.copy_(keyseq[i])
    g.launch()
    if with_keys:
      mjw.reset_data_keyframe(m, de, keyseq[i], masks[i])
    else:
      mjw.reset_data(m, de, masks[i])
    mjw.step(m, de)
  torch.cuda.synchronize()
  assert masks.sum().item() > 8
  for name in ("qpos", "qvel", "time", "history", "act", "mocap_pos", "eq_active"):
    np.testing.assert_array_equal(getattr(dg, name).numpy(), getattr(de, name).numpy(), err_msg=name)
  # the plain graph: unchanged
  plain = mjw.StepGraph(m, dg)
  plain.launch()
  mjw.step(m, de)
  for name in ("qpos", "qvel", "time", "history"):
    np.testing.assert_array_equal(getattr(dg, name).numpy(), getattr(de, name).numpy(), err_msg=name)
  with pytest.raises(ValueError, match="StepGraph"):
    mjw.StepGraph(m, dg, reset=np.ones(W, dtype=bool))  # (the graph reads the mask in place: it must live on the device)
