"""General actuator transmissions: site, site + refsite, ball / free joint and jointinparent targets (csrc/transmission.hpp).

Truth is tests/transmission_truth.py (float64 numpy).  The host tests (structure, acc0, refusals, the truth's own self-check, the
regression on the models that loaded before) run without a GPU; the `gpu` tests compare forward() with the truth fed the device's own
position-stage fields, check the wrench equivalence with xfrc_applied, closed forms on a quadrotor, and determinism of integration.

Finite differences in the self-check: a moment row is the derivative of its length only where the reference's formulation makes it
one -- translational refsite rows in the columns of dofs that move the site itself (or any column when the refsite's frame does not
rotate: the moment ignores the rotation of that frame), and ball-joint rows at the joint's reference orientation (the length is the
rotation vector dotted with the gear; away from the identity its derivative carries the inverse right Jacobian of the exponential map,
which the moment -- the gear itself -- does not).  Rotational refsite lengths are not differentiated for the same reason.
"""

import os
import xml.etree.ElementTree as ET

import numpy as np
import pytest

import conftest
import mujoco_warp_amd as mjw
import transmission_truth as tt
from conftest import relerr
from mujoco_warp_amd import io, mjcf

CHAIN_XML = """
<mujoco>
  <option gravity="0 0 -9.81" timestep="0.002"/>
  <worldbody>
    <site name="anchor" pos=".3 -.2 1"/>
    <body name="b1" pos="0 0 1">
      <joint name="j1" type="hinge" axis="0 1 0"/>
      <geom type="capsule" size=".04" fromto="0 0 0 0 0 -.3" contype="0" conaffinity="0"/>
      <body name="b2" pos="0 0 -.3">
        <joint name="j2" type="hinge" axis="1 0 0"/>
        <geom type="capsule" size=".04" fromto="0 0 0 0 0 -.3" contype="0" conaffinity="0"/>
        <site name="mid" pos=".05 0 -.1" quat=".9 .1 .3 -.2"/>
        <body name="b3" pos="0 0 -.3">
          <joint name="j3" type="slide" axis="0 0 1"/>
          <geom type="sphere" size=".05" contype="0" conaffinity="0"/>
          <body name="b4" pos="0 .05 -.2">
            <joint name="j4" type="ball"/>
            <geom type="capsule" size=".03" fromto="0 0 0 .1 0 -.2" contype="0" conaffinity="0"/>
            <site name="tip" pos=".1 .02 -.2" quat=".8 .2 -.4 .4"/>
          </body>
        </body>
        <body name="fx" pos=".1 .1 0">
          <geom type="sphere" size=".03" contype="0" conaffinity="0"/>
          <site name="fixed" pos="0 .1 .05" quat=".7 0 .7 .1"/>
        </body>
      </body>
    </body>
  </worldbody>
  <actuator>
    <motor name="tip_x" site="tip" gear="1 0 0 0 0 0"/>
    <motor name="tip_rz" site="tip" gear="0 0 0 0 0 1"/>
    <motor name="tip_mixed" site="tip" gear=".3 -1 2 .5 0 -.7"/>
    <motor name="tip_anchor" site="tip" refsite="anchor" gear="1 .5 -2 0 0 0"/>
    <motor name="tip_mid" site="tip" refsite="mid" gear=".3 -1 2 .5 0 -.7"/>
    <motor name="fixed" site="fixed" gear="0 1 0 0 0 .5"/>
    <motor name="anchor" site="anchor" gear="1 0 0 0 0 0"/>
    <motor name="ball" joint="j4" gear="0 1 0"/>
    <general name="ball_parent" jointinparent="j4" gear=".2 1 -.5"/>
  </actuator>
  <sensor>
    <actuatorpos actuator="tip_anchor"/> <actuatorpos actuator="ball"/> <actuatorvel actuator="tip_mixed"/> <actuatorvel actuator="ball_parent"/>
    <actuatorfrc actuator="tip_mid"/> <jointactuatorfrc joint="j1"/> <jointactuatorfrc joint="j3"/>
  </sensor>
</mujoco>
"""

DRONE_XML = """
<mujoco>
  <option gravity="0 0 -9.81" timestep="0.002"/>
  <worldbody>
    <body name="drone" pos="0 0 1">
      <joint name="root" type="free"/>
      <geom type="box" size=".1 .1 .02" mass="1.2" contype="0" conaffinity="0"/>
      <site name="r0" pos=".1 .1 0"/> <site name="r1" pos="-.1 .1 0"/> <site name="r2" pos="-.1 -.1 0"/> <site name="r3" pos=".1 -.1 0"/>
    </body>
  </worldbody>
  <actuator>
    <motor name="m0" site="r0" gear="0 0 1 0 0 .1" ctrlrange="0 10"/>
    <motor name="m1" site="r1" gear="0 0 1 0 0 -.1" ctrlrange="0 10"/>
    <motor name="m2" site="r2" gear="0 0 1 0 0 .1" ctrlrange="0 10"/>
    <motor name="m3" site="r3" gear="0 0 1 0 0 -.1" ctrlrange="0 10"/>
    <motor name="wrench" joint="root" gear="1 2 3 4 5 6"/>
    <general name="wrench_parent" jointinparent="root" gear="1 2 3 4 5 6"/>
  </actuator>
</mujoco>
"""

TWO_ARMS_XML = """
<mujoco>
  <option gravity="0 0 -9.81" timestep="0.002"/>
  <worldbody>
    <body name="a1" pos="-.3 0 1">
      <joint name="ja1" type="hinge" axis="0 1 0"/> <geom type="capsule" size=".03" fromto="0 0 0 .2 0 0" contype="0" conaffinity="0"/>
      <body name="a2" pos=".2 0 0">
        <joint name="ja2" type="hinge" axis="0 0 1"/> <geom type="capsule" size=".03" fromto="0 0 0 .2 0 0" contype="0" conaffinity="0"/>
        <site name="left" pos=".2 0 .02" quat=".9 .2 0 .3"/>
      </body>
    </body>
    <body name="c1" pos=".3 0 1">
      <joint name="jc1" type="hinge" axis="1 0 0"/> <geom type="capsule" size=".03" fromto="0 0 0 0 .2 0" contype="0" conaffinity="0"/>
      <body name="c2" pos="0 .2 0">
        <joint name="jc2" type="hinge" axis="0 1 0"/> <geom type="capsule" size=".03" fromto="0 0 0 0 .2 0" contype="0" conaffinity="0"/>
        <site name="right" pos="0 .2 -.02" quat=".6 0 .5 .6"/>
      </body>
    </body>
  </worldbody>
  <actuator>
    <motor name="between" site="left" refsite="right" gear="1 -2 .5 0 0 0"/>
    <position name="servo" joint="ja2" kp="20" kv="1"/>
  </actuator>
</mujoco>
"""

SMALL = {"chain": CHAIN_XML, "drone": DRONE_XML, "two_arms": TWO_ARMS_XML}
NWORLD = 5
G = 9.81


def _with_site_motor(root, body, gear):
  """a site (offset, rotated) on `body` and a motor on it, appended to the document: the way conftest.multi_humanoid_xml edits the tree"""
  b = next(e for e in root.iter("body") if e.get("name") == body)
  ET.SubElement(b, "site", name="trn_site", pos=".03 -.02 .05", quat=".8 .2 -.4 .4")
  ET.SubElement(root.find("actuator"), "motor", name="trn_motor", site="trn_site", gear=gear)
  return ET.tostring(root, encoding="unicode")


_MODELS = {}


def load(name):
  if name not in _MODELS:
    gear = ".3 -1 2 .5 0 -.7"
    if name in SMALL:
      mjm = mjcf.from_xml_string(SMALL[name])
    elif name == "humanoid":
      mjm = mjcf.from_xml_string(_with_site_motor(ET.parse(conftest.HUMANOID_XML).getroot(), "hand_right", gear), os.path.dirname(conftest.HUMANOID_XML))
    elif name == "three_humanoids":
      mjm = mjcf.from_xml_string(_with_site_motor(ET.fromstring(conftest.multi_humanoid_xml(3)), "hand_right_2", gear), os.path.dirname(conftest.HUMANOID_XML))
    elif name == "g1":
      root, base = ET.parse(conftest.G1_XML).getroot(), os.path.dirname(conftest.G1_XML)
      mjcf._expand_includes(root, base)
      for sec in root.findall("keyframe"):  # (their ctrl vectors have the old actuator count)
        root.remove(sec)
      ET.SubElement(root.find("actuator"), "motor", name="trn_motor", site="right_palm", gear=gear)
      mjm = mjcf.from_xml_string(ET.tostring(root, encoding="unicode"), base)
    _MODELS[name] = mjm
  return _MODELS[name]


def random_state(mjm, nworld, seed=7):
  """distinct qpos (unit quaternions), qvel and ctrl per world; world k is the same whatever nworld"""
  rng = np.random.default_rng(seed)
  qpos = np.tile(np.asarray(mjm.qpos0, dtype=np.float64), (nworld, 1))
  qvel, ctrl = np.zeros((nworld, mjm.nv)), np.zeros((nworld, mjm.nu))
  for w in range(nworld):
    qpos[w] += 0.3 * rng.standard_normal(mjm.nq)
    qvel[w] = 0.5 * rng.standard_normal(mjm.nv)
    ctrl[w] = rng.uniform(-1.0, 1.0, mjm.nu)
  for j in range(mjm.njnt):
    qa, t = int(mjm.jnt_qposadr[j]), int(mjm.jnt_type[j])
    if t in (tt.FREE, tt.BALL):
      qa += 3 if t == tt.FREE else 0
      qpos[:, qa : qa + 4] /= np.linalg.norm(qpos[:, qa : qa + 4], axis=1, keepdims=True)
  return qpos.astype(np.float32), qvel.astype(np.float32), ctrl.astype(np.float32)


def dense(m, d_moment):
  """[nworld, nJmom] sparse rows scattered to [nworld, nu, nv]"""
  rownnz, rowadr, colind = m.moment_rownnz.numpy(), m.moment_rowadr.numpy(), m.moment_colind.numpy()
  out = np.zeros((d_moment.shape[0], m.nu, m.nv), dtype=d_moment.dtype)
  for u in range(m.nu):
    for k in range(rowadr[u], rowadr[u] + rownnz[u]):
      out[:, u, colind[k]] = d_moment[:, k]
  return out


# ----------------------------------------------------------------------------------------------------------------- host
def test_structure_chain():
  mjm = load("chain")
  m = mjw.put_model(mjm)
  site = {n: i for i, n in enumerate(["anchor", "mid", "tip", "fixed"])}  # (the world's own sites first, then the bodies' in document order)
  assert [int(mjm.site_bodyid[site[n]]) for n in ("anchor", "mid", "tip", "fixed")] == [0, 2, 4, 5]
  assert mjm.actuator_trntype.tolist() == [4, 4, 4, 4, 4, 4, 4, 0, 1] and m.actuator_trntype.numpy().tolist() == [4, 4, 4, 4, 4, 4, 4, 0, 1]
  trnid = [[site["tip"], -1]] * 3 + [[site["tip"], site["anchor"]], [site["tip"], site["mid"]], [site["fixed"], -1], [site["anchor"], -1], [3, -1], [3, -1]]
  assert mjm.actuator_trnid.tolist() == trnid and m.actuator_trnid.numpy().tolist() == trnid and m.actuator_trnobj.numpy().tolist() == trnid
  assert m.actuator_gear.numpy()[0, 2].tolist() == pytest.approx([0.3, -1, 2, 0.5, 0, -0.7]) and m.actuator_gear.numpy()[0, 8].tolist() == pytest.approx([0.2, 1, -0.5, 0, 0, 0])
  assert (m.trn_general, m.nJmom, m.nu, m.nv) == (1, 36, 9, 6)
  assert m.moment_rownnz.numpy().tolist() == [6, 6, 6, 6, 4, 2, 0, 3, 3]
  assert m.moment_rowadr.numpy().tolist() == [0, 6, 12, 18, 24, 28, 30, 30, 33]
  full = [0, 1, 2, 3, 4, 5]
  assert m.moment_colind.numpy().tolist() == full * 4 + [2, 3, 4, 5] + [0, 1] + [3, 4, 5] * 2  # (tip - mid: hinges 0 and 1 move both sites)
  assert m.moment_side.numpy().tolist() == [1] * 30 + [0] * 6
  # the transpose: dof-major, actuators ascending
  adr, act, ind = m.momentT_adr.numpy(), m.momentT_act.numpy(), m.momentT_ind.numpy()
  assert adr.tolist() == [0, 5, 10, 15, 22, 29, 36] and act[:5].tolist() == [0, 1, 2, 3, 5] and ind[:5].tolist() == [0, 6, 12, 18, 28]
  assert act[15:22].tolist() == [0, 1, 2, 3, 4, 7, 8] and ind[15:22].tolist() == [3, 9, 15, 21, 25, 30, 33]
  # Data: the reference's schema, filled once
  d = mjw.make_data(mjm, nworld=3)
  assert d.actuator_moment.shape == (3, 36) and d.moment_colind.shape == (3, 36) and d.moment_rownnz.shape == (3, 9)
  assert (d.moment_rowadr.numpy() == m.moment_rowadr.numpy()).all() and (d.moment_colind.numpy()[2] == m.moment_colind.numpy()).all()
  # what the single-dof kernels index with is always a joint
  assert m.actuator_trnjnt.numpy()[:, 0].tolist() == [0, 0, 0, 0, 2, 0, 0, 3, 3] and io.c_model(m).actuator_trnid == m.actuator_trnjnt.ptr


def test_structure_drone_and_two_arms():
  mjm = load("drone")
  m = mjw.put_model(mjm)
  assert mjm.actuator_trntype.tolist() == [4, 4, 4, 4, 0, 1] and mjm.actuator_trnid.tolist() == [[0, -1], [1, -1], [2, -1], [3, -1], [0, -1], [0, -1]]
  gear = np.array([[0, 0, 1, 0, 0, 0.1], [0, 0, 1, 0, 0, -0.1], [0, 0, 1, 0, 0, 0.1], [0, 0, 1, 0, 0, -0.1], [1, 2, 3, 4, 5, 6], [1, 2, 3, 4, 5, 6]], dtype=np.float32)
  assert (m.actuator_gear.numpy()[0] == gear).all()
  assert (m.trn_general, m.nJmom) == (1, 36) and m.moment_rownnz.numpy().tolist() == [6] * 6 and m.moment_rowadr.numpy().tolist() == [0, 6, 12, 18, 24, 30]
  assert m.moment_colind.numpy().tolist() == [0, 1, 2, 3, 4, 5] * 6 and m.moment_side.numpy().tolist() == [1] * 24 + [0] * 12
  assert m.actuator_ctrllimited.numpy().tolist() == [1, 1, 1, 1, 0, 0]
  mjm = load("two_arms")
  m = mjw.put_model(mjm)
  assert mjm.actuator_trntype.tolist() == [4, 0] and mjm.actuator_trnid.tolist() == [[0, 1], [1, -1]]
  assert (m.trn_general, m.nJmom) == (1, 5) and m.moment_rownnz.numpy().tolist() == [4, 1] and m.moment_rowadr.numpy().tolist() == [0, 4]
  assert m.moment_colind.numpy().tolist() == [0, 1, 2, 3, 1] and m.moment_side.numpy().tolist() == [1, 1, 2, 2, 0]  # the union of both chains
  assert (m.act_dof_max, m.act_velfeedback) == (1, 0) and m.actuator_trnjnt.numpy().tolist() == [[0, -1], [1, -1]]  # (_act_limits: the single-dof row only)
  # every tree that owns a column of a row never sleeps
  assert mjm.tree_sleep_policy.tolist() == [1, 1]


@pytest.mark.parametrize("name", list(SMALL))
def test_acc0(name):
  mjm = load(name)
  _, moment = tt.truth_host(mjm, mjm.qpos0)
  Minv = np.linalg.inv(mjcf.host_mass_matrix(mjm, mjm.qpos0)["M"])
  for u in range(mjm.nu):
    assert abs(mjm.actuator_acc0[u] - np.linalg.norm(Minv @ moment[u])) <= 1e-12, (name, u)


def _one(actuator, option=""):
  return f"""<mujoco>{option}<worldbody><site name="w"/><body name="b"><joint name="j" type="ball"/><geom size=".1"/><site name="s"/>
    <body name="c" pos="0 0 .3"><joint name="h" type="hinge"/><geom size=".1"/><site name="t"/></body></body></worldbody>
    <actuator>{actuator}</actuator></mujoco>"""


def test_refusals():
  for act, word in (('<general body="b"/>', "body"), ('<general cranksite="s" slidersite="t" cranklength=".1"/>', "slider-crank"), ('<general tendon="ten"/>', "tendon")):
    with pytest.raises(NotImplementedError, match=f"{word}.*not built"):
      mjcf.from_xml_string(_one(act))
  for trntype, word in ((2, "slider-crank"), (3, "tendon"), (5, "body")):  # ... and from a compiled model
    mjm = mjcf.from_xml_string(DRONE_XML)
    mjm.actuator_trntype[0] = trntype
    with pytest.raises(NotImplementedError, match=f"{word}.*not built"):
      mjw.put_model(mjm)
  plain = _one("X")
  for act in ('<motor name="two" joint="h" site="s"/>', '<motor name="two" joint="h" jointinparent="j"/>', '<motor name="none"/>', '<motor name="two" joint="h" refsite="s"/>'):
    with pytest.raises(ValueError, match="actuator 0 '(two|none)'"):
      mjcf.from_xml_string(plain.replace("X", act))
  for act in ('<motor name="lost" site="nowhere"/>', '<motor name="lost" site="s" refsite="nowhere"/>', '<motor name="lost" jointinparent="nowhere"/>'):
    with pytest.raises(ValueError, match="actuator 0 'lost'.*nowhere"):
      mjcf.from_xml_string(plain.replace("X", act))
  # velocity feedback on a multi-dof row: the implicit integrators refuse it, Euler and RK4 take it; without feedback all four load
  for integrator in ("implicitfast", "implicit", "Euler", "RK4"):
    opt = f'<option integrator="{integrator}"/>'
    for act in ('<velocity site="t" kv="2" gear="1 0 0 0 0 0"/>', '<position joint="j" kp="3" kv="1" gear="1 0 0"/>', '<general site="s" gaintype="affine" gainprm="1 0 .5"/>'):
      mjm = mjcf.from_xml_string(plain.replace("X", act).replace("<mujoco>", "<mujoco>" + opt))
      if integrator.startswith("implicit"):
        with pytest.raises(NotImplementedError, match=f"velocity feedback.*multi-dof.*{integrator}"):
          mjw.put_model(mjm)
      else:
        m = mjw.put_model(mjm)
        assert m.trn_general == 1 and io.c_model(m).integrator == int(m.opt.integrator)
        m.opt.integrator = int(mjw.IntegratorType.IMPLICITFAST)  # (read live when the C struct is rebuilt)
        with pytest.raises(NotImplementedError, match="velocity feedback.*multi-dof.*implicitfast"):
          io.c_model(m)
    for act in ('<motor site="t" gear="1 0 0 0 0 0"/>', '<position joint="j" kp="3" gear="1 0 0"/><velocity joint="h" kv="2"/>'):
      m = mjw.put_model(mjcf.from_xml_string(plain.replace("X", act).replace("<mujoco>", "<mujoco>" + opt)))
      assert m.trn_general == 1 and m.act_dof_max == (1 if "velocity" in act else 0)


@pytest.mark.parametrize("name", list(SMALL))
def test_truth_self_check(name):
  mjm = load(name)
  qpos = random_state(mjm, 3)[0].astype(np.float64)
  trnid = np.asarray(mjm.actuator_trnid).reshape(-1, 2)
  for w in range(3):
    q = qpos[w].copy()
    for j in range(mjm.njnt):  # ball joints at their reference orientation (module docstring); everything else stays random
      if int(mjm.jnt_type[j]) == tt.BALL:
        q[int(mjm.jnt_qposadr[j]) : int(mjm.jnt_qposadr[j]) + 4] = [1, 0, 0, 0]
    length, moment = tt.truth_host(mjm, q)
    checked = 0
    for u in range(mjm.nu):
      t, (id0, id1), g = int(mjm.actuator_trntype[u]), trnid[u], np.asarray(mjm.actuator_gear[u], dtype=np.float64)
      ball = t in (0, 1) and int(mjm.jnt_type[id0]) == tt.BALL
      transl_ref = t == 4 and id1 >= 0 and not g[3:].any()
      if ball or transl_ref:
        own = set(tt._moving(mjm, int(mjm.site_bodyid[id0]))) if transl_ref else None
        fixed_ref = transl_ref and int(mjm.body_weldid[int(mjm.site_bodyid[id1])]) == 0
        for i in range(mjm.nv):
          if transl_ref and not (fixed_ref or (i in own and moment[u, i] != 0.0)):
            continue
          h = 1e-6
          fd = (tt.truth_host(mjm, tt.advance(mjm, q, i, h))[0][u] - tt.truth_host(mjm, tt.advance(mjm, q, i, -h))[0][u]) / (2 * h)
          assert abs(fd - moment[u, i]) <= 1e-7, (name, w, u, i, fd, moment[u, i])
          checked += 1
      if t == 4 and id1 < 0:  # moment' f == J' (wrench f) against the Jacobian written from anchors and axes
        hf = tt.host_fields(mjm, q)
        jp, jr = tt.body_jacobian(mjm, q, hf["site_xpos"][id0], int(mjm.site_bodyid[id0]))
        f = 1.7
        want = jp.T @ (hf["site_xmat"][id0] @ g[:3] * f) + jr.T @ (hf["site_xmat"][id0] @ g[3:] * f)
        assert np.abs(moment[u] * f - want).max() <= 1e-12, (name, w, u)
        checked += 1
    assert checked > 0


def test_models_that_loaded_before_are_unchanged(humanoid):
  for mjm in (mjcf.from_xml_string(conftest.PENDULA_XML), humanoid, mjcf.load_xml(conftest.G1_XML)):
    m = mjw.put_model(mjm)
    assert m.trn_general == 0 and m.nJmom == m.nu and (m.moment_rownnz.numpy() == 1).all()
    assert (m.moment_colind.numpy() == np.asarray(mjm.jnt_dofadr)[np.asarray(mjm.actuator_trnid).reshape(-1, 2)[:, 0]]).all()
    assert io.c_model(m).actuator_trnid == m.actuator_trnid.ptr and io.c_model(m).trn_general == 0
    assert mjw.make_data(mjm, nworld=2).actuator_moment.shape == (2, m.nu)


def test_lane_class_models_load():
  for name, nv in (("humanoid", 27), ("g1", 35), ("three_humanoids", 81)):
    mjm = load(name)
    m = mjw.put_model(mjm)
    assert mjm.nv == nv and m.trn_general == 1 and m.nJmom > m.nu and int(mjm.actuator_trntype[-1]) == 4
    chain = m.moment_colind.numpy()[m.moment_rowadr.numpy()[-1] :]
    assert chain.tolist() == tt._moving(mjm, int(mjm.site_bodyid[int(mjm.actuator_trnid[-1, 0])]))


# ------------------------------------------------------------------------------------------------------------------ gpu
def _forward(name, nworld, integrator=None):
  mjm = load(name)
  if integrator is not None:
    mjm = mjcf.from_xml_string(SMALL[name].replace("<option ", f'<option integrator="{integrator}" '))
  m = mjw.put_model(mjm)
  d = mjw.make_data(mjm, nworld=nworld)
  qpos, qvel, ctrl = random_state(mjm, nworld)
  d.qpos.assign(qpos)
  d.qvel.assign(qvel)
  d.ctrl.assign(ctrl)
  return mjm, m, d


@pytest.mark.gpu
@pytest.mark.parametrize("name,nworld", [("chain", NWORLD), ("chain", 67), ("drone", NWORLD), ("two_arms", NWORLD), ("humanoid", NWORLD), ("g1", NWORLD), ("three_humanoids", NWORLD)])
def test_forward_against_truth(name, nworld):
  mjm, m, d = _forward(name, nworld)
  mjw.forward(m, d)
  qpos, qvel = d.qpos.numpy(), d.qvel.numpy().astype(np.float64)
  length, moment = d.actuator_length.numpy(), dense(m, d.actuator_moment.numpy())
  velocity, force, qfrc = d.actuator_velocity.numpy(), d.actuator_force.numpy().astype(np.float64), d.qfrc_actuator.numpy()
  fields = [getattr(d, f).numpy() for f in ("site_xpos", "site_xmat", "xquat", "subtree_com", "cdof")]
  worst = np.zeros(4)
  for w in range(nworld):
    want_len, want_mom = tt.truth(mjm, qpos[w], *(f[w] for f in fields))
    assert (moment[w][want_mom == 0.0] == 0.0).all(), (name, w)  # structural zeros are exact
    errs = (relerr(length[w], want_len) if np.abs(want_len).max() > 0 else float(np.abs(length[w]).max()), relerr(moment[w], want_mom),
            relerr(velocity[w], moment[w].astype(np.float64) @ qvel[w]), float(np.abs(qfrc[w] - moment[w].astype(np.float64).T @ force[w]).max()))
    worst = np.maximum(worst, errs)
  print(f"{name} x{nworld}: length {worst[0]:.2e} moment {worst[1]:.2e} velocity {worst[2]:.2e} qfrc_actuator {worst[3]:.2e}")
  assert worst[0] <= 2e-5 and worst[1] <= 2e-5 and worst[2] <= 2e-5 and worst[3] <= 1e-4, worst
  assert np.abs(force).max() > 0 and np.abs(qfrc).max() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["chain", "drone", "humanoid"])
def test_wrench_equivalence(name):
  """ctrl on a site actuator == the same wrench as xfrc_applied on the site's body (a path this feature does not touch)"""
  mjm, m, d = _forward(name, NWORLD)
  trnid = np.asarray(mjm.actuator_trnid).reshape(-1, 2)
  ids = [u for u in range(mjm.nu) if int(mjm.actuator_trntype[u]) == 4 and trnid[u, 1] < 0]
  assert ids
  state = [d.qpos.numpy().copy(), d.qvel.numpy().copy()]
  for u in ids:
    ctrl = np.zeros((NWORLD, mjm.nu), dtype=np.float32)
    ctrl[:, u] = np.linspace(0.5, 2.5, NWORLD)
    d.ctrl.assign(ctrl)
    d.xfrc_applied.assign(np.zeros((NWORLD, mjm.nbody, 6), dtype=np.float32))
    mjw.forward(m, d)
    a, f = d.qfrc_smooth.numpy().copy(), d.actuator_force.numpy()[:, u].astype(np.float64)
    s, b = int(trnid[u, 0]), int(mjm.site_bodyid[int(trnid[u, 0])])
    xmat, xpos, xipos = d.site_xmat.numpy()[:, s].astype(np.float64), d.site_xpos.numpy()[:, s].astype(np.float64), d.xipos.numpy()[:, b].astype(np.float64)
    g = np.asarray(mjm.actuator_gear[u], dtype=np.float64)
    xfrc = np.zeros((NWORLD, mjm.nbody, 6))
    for w in range(NWORLD):
      force = xmat[w] @ g[:3] * f[w]
      xfrc[w, b, :3], xfrc[w, b, 3:] = force, xmat[w] @ g[3:] * f[w] + np.cross(xpos[w] - xipos[w], force)
    d.ctrl.assign(np.zeros_like(ctrl))
    d.xfrc_applied.assign(xfrc.astype(np.float32))
    mjw.forward(m, d)
    err = np.abs(d.qfrc_smooth.numpy() - a).max()
    assert (d.qpos.numpy() == state[0]).all() and err <= 1e-4, (name, u, err)
    if b > 0 and int(mjm.body_weldid[b]) > 0:
      assert np.abs(a - _baseline(m, d, mjm)).max() > 1e-3  # (the actuator did something)


def _baseline(m, d, mjm):
  d.xfrc_applied.assign(np.zeros((d.nworld, mjm.nbody, 6), dtype=np.float32))
  mjw.forward(m, d)
  return d.qfrc_smooth.numpy().copy()


@pytest.mark.gpu
def test_drone_closed_forms():
  mjm = load("drone")
  m = mjw.put_model(mjm)
  d = mjw.make_data(mjm, nworld=NWORLD)
  qpos = random_state(mjm, NWORLD)[0]
  d.qpos.assign(qpos)
  mass = float(mjm.body_mass[1])
  assert mass == pytest.approx(1.2)
  R = np.array([tt.qmat(tt.qnorm(q[3:7])) for q in qpos.astype(np.float64)])
  ctrl = np.zeros((NWORLD, mjm.nu), dtype=np.float32)
  ctrl[:, :4] = mass * G / 4
  d.ctrl.assign(ctrl)
  mjw.forward(m, d)
  # hover thrust along the body z axis: in the world frame the net linear acceleration is (R z - z) g; level worlds hover
  lin = d.qacc.numpy()[:, :3].astype(np.float64)
  assert np.abs(lin - (R[:, :, 2] - [0, 0, 1]) * G).max() <= 1e-4 * G
  level = np.tile(np.asarray(mjm.qpos0, dtype=np.float32), (NWORLD, 1))
  level[:, :3] = qpos[:, :3]
  d.qpos.assign(level)
  mjw.forward(m, d)
  assert np.abs(d.qacc.numpy()[:, :3]).max() <= 1e-4 * G
  d.qpos.assign(qpos)
  ctrl[:] = 0
  ctrl[:, 2] = np.linspace(1, 5, NWORLD)
  d.ctrl.assign(ctrl)
  mjw.forward(m, d)
  want = R[:, :, 2] * (ctrl[:, 2:3].astype(np.float64) / mass) + [0, 0, -G]
  assert np.abs(d.qacc.numpy()[:, :3] - want).max() <= 1e-4


@pytest.mark.gpu
@pytest.mark.parametrize("integrator", ["Euler", "RK4", "implicitfast"])
@pytest.mark.parametrize("name", ["drone", "chain"])
def test_integration_is_deterministic(name, integrator):
  import torch

  runs = {}
  for key, nworld, graph in (("a", NWORLD, False), ("b", NWORLD, False), ("wide", 67, False), ("graph", NWORLD, True)):
    mjm, m, d = _forward(name, nworld, integrator)
    g = mjw.StepGraph(m, d) if graph else None
    for _ in range(20):
      g.launch() if graph else mjw.step(m, d)
    torch.cuda.synchronize()
    runs[key] = [getattr(d, f).numpy().copy() for f in ("qpos", "qvel", "qfrc_actuator", "actuator_moment", "actuator_velocity")]
  assert np.isfinite(runs["a"][0]).all() and not any(np.isnan(x).any() for x in runs["a"])
  assert np.abs(runs["a"][0] - random_state(load(name), NWORLD)[0]).max() > 1e-4  # (it moved)
  for key in ("b", "wide", "graph"):
    for x, y in zip(runs["a"], runs[key]):
      assert (x == y[:NWORLD]).all(), (name, integrator, key)


@pytest.mark.gpu
def test_sensors_read_the_data_fields():
  mjm, m, d = _forward("chain", NWORLD)
  mjw.forward(m, d)
  s = d.sensordata.numpy()
  names = list(mjm.actuator_names)
  u = {n: names.index(n) for n in names}
  want = np.stack([d.actuator_length.numpy()[:, u["tip_anchor"]], d.actuator_length.numpy()[:, u["ball"]], d.actuator_velocity.numpy()[:, u["tip_mixed"]],
                   d.actuator_velocity.numpy()[:, u["ball_parent"]], d.actuator_force.numpy()[:, u["tip_mid"]], d.qfrc_actuator.numpy()[:, 0],
                   d.qfrc_actuator.numpy()[:, 2]], axis=1)
  assert s.shape == want.shape and (s == want).all() and np.abs(want).min() > 0
