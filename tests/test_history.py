"""Actuator and sensor delays (csrc/history.hpp): loader, layout, refusals, state, and the kernels against tests/history_truth.py.

The truth is float64 Python.  Zero-order hold returns stored samples, so those comparisons are bitwise; interpolated reads are compared with
the truth fed the device's own float32 query time and buffer (read back), so that only the ~20 float32 operations of the interpolation differ:
bound 32 float32 ulps of max |value| in the buffer.  A delayed sensor is checked against an undelayed twin of the same sensor in the same
model, whose reading is the fresh value the delayed one stored.
"""

import numpy as np
import pytest

import history_truth as ht
import mujoco_warp_amd as mjw
from mujoco_warp_amd import io, mjcf

ULP32 = 2.0 ** -23
INTEGRATION = int(mjw.State.INTEGRATION)


def slide_xml(actuators="", sensors="", integrator="Euler", njoint=1, option="", default=""):
  bodies = "".join(f'<body pos="0 {k} 0"><joint name="j{k}" type="slide" axis="1 0 0"/><geom size=".1" mass="1"/><site name="s{k}"/></body>' for k in range(njoint))
  return (f'<mujoco><option timestep="0.01" integrator="{integrator}">{option}</option>{default}<worldbody>{bodies}</worldbody>'
          f'<actuator>{actuators}</actuator><sensor>{sensors}</sensor></mujoco>')


BALL_XML = """
<mujoco><option timestep="0.01" gravity="0 0 0"/>
<worldbody><body><joint name="b" type="ball"/><geom type="box" size=".1 .2 .3" mass="1"/></body></worldbody>
<sensor>
  <ballquat joint="b"/><ballangvel joint="b"/>
  <ballquat joint="b" delay="{d}" nsample="{n}"/><ballangvel joint="b" delay="{d}" nsample="{n}"/>
</sensor></mujoco>
"""


# ----------------------------------------------------------------------------------------------------------------- the truth's own checks
def test_truth_zoh_delay_shifts_the_input_by_k_steps():
  dt = 0.01
  for k, n in ((2, 2), (4, 5), (1, 1), (3, 7)):
    buf, x = ht.Buffer.initial(n, 1, 0.0, dt), [float(i * i + 1) for i in range(15)]
    out = [ht.evaluate(buf, i * dt, k * dt, ht.ZOH, x[i], True)[0] for i in range(15)]
    assert out == [0.0] * k + x[: 15 - k]


def test_truth_linear_reproduces_a_ramp_and_cubic_a_quadratic():
  n, dt = 8, 0.01
  buf = ht.Buffer(n, 2)
  for i in range(11):  # (wraps: the ring is not in physical order)
    buf.insert(i * dt, [3.0 * i * dt - 1.0, (i * dt) ** 2])
  lt = buf.logical_times()
  np.testing.assert_allclose(lt, np.arange(3, 11) * dt, atol=1e-15)
  for t in np.linspace(lt[0], lt[-1], 57):
    assert abs(buf.read(t, ht.LINEAR)[0] - (3.0 * t - 1.0)) < 1e-12
    if lt[1] <= t <= lt[-2]:  # interior spans: both Catmull-Rom slopes are central differences, exact for a quadratic on a uniform grid
      assert abs(buf.read(t, ht.CUBIC)[1] - t * t) < 1e-12
  assert buf.read(lt[0] - 1.0, ht.CUBIC)[0] == buf.logical_values()[0][0] and buf.read(lt[-1] + 1.0, ht.LINEAR)[1] == buf.logical_values()[-1][1]


def test_truth_out_of_order_insert_keeps_times_sorted():
  rng = np.random.default_rng(0)
  buf = ht.Buffer(5, 1)
  buf.times = np.arange(-5, 0) * 0.01
  buf.values = buf.times.reshape(5, 1).copy()  # (every sample's value is its time)
  for t in rng.uniform(-0.1, 0.3, 60):
    before = buf.logical_times()
    buf.insert(float(t), [t])
    lt = buf.logical_times()
    assert (np.diff(lt) > 0).all() and (buf.logical_values()[:, 0] == lt).all()
    if before[0] < t < before[-1] and np.abs(before - t).min() >= ht.EPS:
      assert t in lt and before[0] not in lt and (lt[-1], len(lt)) == (before[-1], 5)  # in between: the oldest sample made room
  lt = buf.logical_times()
  buf.insert(float(lt[2]), [7.0])  # exact match: overwritten in place
  assert (buf.logical_times() == lt).all() and buf.logical_values()[2, 0] == 7.0


# ----------------------------------------------------------------------------------------------------------------- loader and layout (CPU)
def test_loader_reads_delay_nsample_interp_and_defaults_classes():
  xml = slide_xml(
    default='<default><general delay="0.03" nsample="4" interp="linear"/><default class="fast"><motor delay="0.01" nsample="2"/></default></default>',
    actuators='<motor name="a0" joint="j0"/><motor name="a1" joint="j1" class="fast"/><position name="a2" joint="j0" delay="0" nsample="3" interp="cubic"/>'
              '<general name="a3" joint="j1" nsample="0" delay="0"/>',
    sensors='<jointpos joint="j0"/><jointvel joint="j1" delay="0.02" nsample="3" interp="cubic"/><framepos objtype="site" objname="s0" nsample="2"/>'
            '<accelerometer site="s1" delay="0.05" nsample="6" interp="linear"/>', njoint=2)
  m = mjcf.from_xml_string(xml)
  assert m.actuator_history.tolist() == [[4, 1], [2, 1], [3, 2], [0, 1]]
  np.testing.assert_allclose(m.actuator_delay, [0.03, 0.01, 0.0, 0.0])
  assert m.sensor_history.tolist() == [[0, 0], [3, 2], [2, 0], [6, 1]] and m.sensor_interval.shape == (4, 2) and not m.sensor_interval.any()
  np.testing.assert_allclose(m.sensor_delay, [0.0, 0.02, 0.0, 0.05])
  # [user, cursor, times[n], values[n * dim]] per buffer: actuators first, then sensors, in id order
  assert m.actuator_historyadr.tolist() == [0, 10, 16, -1]
  assert m.sensor_historyadr.tolist() == [-1, 24, 32, 42] and m.nhistory == 42 + 2 + 6 * 4
  d = mjcf.MjData(m)
  assert d.history.shape == (m.nhistory,)
  b = ht.Buffer.from_flat(d.history, 32, 2, 3)
  assert b.cursor == 1 and b.user == 0.0 and not b.values.any()
  np.testing.assert_allclose(b.times, [-0.02, -0.01])
  with pytest.raises(ValueError, match="interp"):
    mjcf.from_xml_string(slide_xml(actuators='<motor joint="j0" nsample="2" interp="spline"/>'))


def test_put_model_tables_and_stage_lists():
  xml = slide_xml(actuators='<motor name="a0" joint="j0" delay="0.02" nsample="2"/><motor name="a1" joint="j0"/>',
                  sensors='<accelerometer site="s0" delay="0.01" nsample="1"/><jointpos joint="j0"/><actuatorfrc actuator="a0" delay="0.01" nsample="2"/>'
                          '<jointvel joint="j0" nsample="3"/><touch site="s0" nsample="2"/>')
  mjm = mjcf.from_xml_string(xml)
  m = mjw.put_model(mjm)
  assert (m.nhistory, m.nu_history, m.nsensor_history_posvel, m.nsensor_history_acc) == (mjm.nhistory, 1, 2, 2)
  # the lists follow the two sensor launches: accelerometer and touch are written behind the solver, everything else (actuator forces too) before it
  assert m.sensor_history_posvel.numpy().tolist() == [2, 3, -1, -1, -1] and m.sensor_history_acc.numpy().tolist() == [0, 4, -1, -1, -1]
  assert m.actuator_history.numpy().tolist() == [[2, 0], [0, 0]] and m.actuator_historyadr.numpy().tolist() == [0, -1]
  np.testing.assert_array_equal(m.sensor_historyadr.numpy(), mjm.sensor_historyadr)
  assert m.sensor_interval.shape == (5, 2) and m.sensor_delay.numpy().dtype == np.float32
  c = io.c_model(m)
  assert (c.nhistory, c.nu_history, c.nsensor_history_posvel, c.nsensor_history_acc) == (mjm.nhistory, 1, 2, 2) and c.sensor_history_acc != 0
  d = mjw.make_data(mjm, nworld=3)
  assert d.history.shape == (3, mjm.nhistory) and d.ws_ctrl_delayed.shape == (3, 2)
  np.testing.assert_array_equal(d.history.numpy(), np.tile(mjcf.MjData(mjm).history.astype(np.float32), (3, 1)))
  # put_data: the host's buffers verbatim
  mjd = mjcf.MjData(mjm)
  mjd.history[:] = np.arange(mjm.nhistory) * 0.5
  np.testing.assert_array_equal(mjw.put_data(mjm, mjd, nworld=2).history.numpy(), np.tile(mjd.history.astype(np.float32), (2, 1)))
  out = mjcf.MjData(mjm)
  mjw.get_data_into(out, mjm, mjw.put_data(mjm, mjd, nworld=2), 1)
  np.testing.assert_array_equal(out.history, mjd.history)


def test_refusals_interval_sleep_and_delay_without_samples():
  with pytest.raises(NotImplementedError, match=r"(?s)'slow'.*interval"):
    mjcf.from_xml_string(slide_xml(sensors='<jointpos name="slow" joint="j0" interval="0.05"/>'))
  with pytest.raises(ValueError, match="nsample"):
    mjcf.from_xml_string(slide_xml(actuators='<motor joint="j0" delay="0.02"/>'))
  with pytest.raises(ValueError, match="nsample"):
    mjcf.from_xml_string(slide_xml(sensors='<jointpos joint="j0" delay="0.02"/>'))
  # ... and put_model says the same to a compiled model that carries them
  mjm = mjcf.from_xml_string(slide_xml(sensors='<jointpos name="slow" joint="j0" nsample="2"/>'))
  mjm.sensor_interval = np.array([[0.05, 0.0]])
  with pytest.raises(NotImplementedError, match=r"(?s)'slow'.*interval"):
    mjw.put_model(mjm)
  mjm = mjcf.from_xml_string(slide_xml(actuators='<motor joint="j0" nsample="2"/>'))
  mjm.actuator_delay = np.array([0.02])
  mjm.actuator_history = np.array([[0, 0]])
  mjm.actuator_historyadr, mjm.nhistory = np.array([-1]), 0
  with pytest.raises(ValueError, match="nsample"):
    mjw.put_model(mjm)
  sleepy = mjcf.from_xml_string(slide_xml(actuators='<motor joint="j0" delay="0.02" nsample="2"/>', option='<flag sleep="enable"/>'))
  sleepy.opt.solver = int(mjw.SolverType.NEWTON)
  with pytest.raises(NotImplementedError, match="sleep"):
    mjw.put_model(sleepy)
  sleepy.actuator_history[:], sleepy.actuator_delay[:], sleepy.actuator_historyadr[:], sleepy.nhistory = 0, 0.0, -1, 0
  assert mjw.put_model(sleepy).nhistory == 0  # (sleeping alone still loads)


class _Without:
  """The wrapped host model minus the history names: an object that predates them."""

  def __init__(self, obj):
    object.__setattr__(self, "_obj", obj)

  def __getattr__(self, k):
    if k in ("actuator_history", "actuator_historyadr", "actuator_delay", "sensor_history", "sensor_historyadr", "sensor_delay", "sensor_interval", "nhistory"):
      raise AttributeError(k)
    return getattr(self._obj, k)


def test_a_model_without_the_history_names_has_no_history():
  mjm = mjcf.from_xml_string(slide_xml(actuators='<motor joint="j0" delay="0.02" nsample="2"/>', sensors='<jointpos joint="j0" nsample="2"/>'))
  m = mjw.put_model(_Without(mjm))
  assert (m.nhistory, m.nu_history, m.nsensor_history_posvel, m.nsensor_history_acc) == (0, 0, 0, 0)
  assert m.actuator_history.numpy().tolist() == [[0, 0]] and m.sensor_historyadr.numpy().tolist() == [-1]
  d = mjw.make_data(m, nworld=2)
  assert d.history.shape == (2, 0) and io.c_data(d).history in (0, None)


def test_state_size_counts_history_in_enum_order():
  plain = mjw.put_model(mjcf.from_xml_string(slide_xml(actuators='<motor joint="j0"/>', sensors='<jointpos joint="j0"/>')))
  mjm = mjcf.from_xml_string(slide_xml(actuators='<motor joint="j0" delay="0.02" nsample="2"/>', sensors='<jointpos joint="j0" nsample="3"/>'))
  m = mjw.put_model(mjm)
  S = mjw.State
  assert mjw.state_size(plain, INTEGRATION) == 1 + 1 + 1 + 0 + 1 + 1 + 1 + 12  # time qpos qvel act warmstart ctrl qfrc_applied xfrc_applied: as before
  assert mjw.state_size(plain, int(S.HISTORY)) == 0
  assert mjw.state_size(m, int(S.HISTORY)) == mjm.nhistory == 6 + 8
  assert mjw.state_size(m, INTEGRATION) == mjw.state_size(plain, INTEGRATION) + mjm.nhistory
  assert mjw.state_size(m, int(S.PHYSICS)) == 3 + mjm.nhistory
  d = mjw.make_data(mjm, nworld=2)
  fields = io._state_fields(m, d, int(S.ACT | S.HISTORY | S.WARMSTART | S.QVEL))
  assert [n for _, n in fields] == [1, mjm.nhistory, 1] and fields[1][0] is d.history  # (qvel, history, warmstart: the enum's order; na = 0)


def test_init_history_refuses_times_that_do_not_increase():
  mjm = mjcf.from_xml_string(slide_xml(actuators='<motor joint="j0" delay="0.02" nsample="3"/>', sensors='<jointpos joint="j0" nsample="3"/>'))
  m, d = mjw.put_model(mjm), mjw.make_data(mjm, nworld=2)
  vals, phase = mjw.DeviceArray.zeros((2, 3)), mjw.DeviceArray.zeros((2,))
  for bad in ([0.0, 0.01, 0.01], [0.0, 0.02, 0.01]):
    times = mjw.DeviceArray.from_numpy(np.array(bad, dtype=np.float32))
    with pytest.raises(ValueError, match="strictly increasing"):
      mjw.init_ctrl_history(m, d, 0, times, vals)
    with pytest.raises(ValueError, match="strictly increasing"):
      mjw.init_sensor_history(m, d, 0, times, vals, phase)
  with pytest.raises(ValueError, match="out of range"):
    mjw.init_ctrl_history(m, d, 1, None, vals)


# ----------------------------------------------------------------------------------------------------------------- GPU
def _buffers(mjm):
  """{("act" | "sens", id): (adr, n, dim, interp, delay)} of the host model's buffers."""
  out = {}
  for kind, hist, adr, delay, dims in (("act", mjm.actuator_history, mjm.actuator_historyadr, mjm.actuator_delay, np.ones(mjm.nu, dtype=int)),
                                       ("sens", mjm.sensor_history, mjm.sensor_historyadr, mjm.sensor_delay, mjm.sensor_dim)):
    for i in range(len(hist)):
      if hist[i, 0] > 0:
        out[(kind, i)] = (int(adr[i]), int(hist[i, 0]), int(dims[i]), int(hist[i, 1]), float(np.float32(delay[i])))
  return out


def _ctrl_seq(nworld, nstep, nu=1):
  rng = np.random.default_rng(7)
  return rng.uniform(-2.0, 2.0, (nstep, 8, nu)).astype(np.float32)[:, :nworld]  # (world w's sequence does not depend on nworld)


def _run_actuator(mjm, nworld, nstep, ctrl, use_graph=False):
  """Steps with ctrl[i] set before step i; returns (actuator_force after every step, Data.time before it, Data.history after it, d)."""
  m, d = mjw.put_model(mjm), mjw.make_data(mjm, nworld=nworld)
  graph = mjw.StepGraph(m, d) if use_graph else None
  force, times, hist = [], [], []
  for i in range(nstep):
    d.ctrl.assign(ctrl[i])
    times.append(d.time.numpy().copy())
    graph.launch() if graph else mjw.step(m, d)
    force.append(d.actuator_force.numpy().copy())
    hist.append(d.history.numpy().copy())
  return np.array(force), np.array(times), np.array(hist), d


def _truth_actuator(mjm, times, ctrl, nworld, u=0):
  adr, n, dim, interp, delay = _buffers(mjm)[("act", u)]
  out = np.zeros((len(times), nworld))
  for w in range(nworld):
    buf = ht.Buffer.initial(n, 1, 0.0, np.float32(0.01))
    buf.times = buf.times.astype(np.float32).astype(np.float64)
    for i in range(len(times)):
      out[i, w] = ht.evaluate(buf, float(times[i][w]), delay, interp, ctrl[i][w][u], True)[0]
  return out


@pytest.mark.gpu
@pytest.mark.parametrize("nworld", [1, 3])
@pytest.mark.parametrize("delay,nsample", [(0.02, 2), (0.04, 5)])
def test_actuator_delay_zoh_is_bitwise_the_ctrl_of_delay_ago(delay, nsample, nworld):
  mjm = mjcf.from_xml_string(slide_xml(actuators=f'<motor joint="j0" delay="{delay}" nsample="{nsample}"/>'))
  ctrl, k = _ctrl_seq(nworld, 12), round(delay / 0.01)
  force, times, hist, _ = _run_actuator(mjm, nworld, 12, ctrl)
  assert (force[:k] == 0).all()
  np.testing.assert_array_equal(force[k:, :, 0], ctrl[: 12 - k, :, 0])
  np.testing.assert_array_equal(force[:, :, 0], _truth_actuator(mjm, times, ctrl, nworld))
  # hipGraph replay: bitwise the eager run
  gforce, _, ghist, _ = _run_actuator(mjm, nworld, 12, ctrl, use_graph=True)
  np.testing.assert_array_equal(gforce, force)
  np.testing.assert_array_equal(ghist, hist)


@pytest.mark.gpu
@pytest.mark.parametrize("delay,nsample", [(0.02, 2), (0.04, 5)])
def test_rk4_inserts_one_sample_per_step(delay, nsample):
  mjm = mjcf.from_xml_string(slide_xml(actuators=f'<motor joint="j0" delay="{delay}" nsample="{nsample}"/>', sensors='<jointvel joint="j0" nsample="6"/>', integrator="RK4"))
  nworld, ctrl = 2, _ctrl_seq(2, 12)
  force, times, hist, _ = _run_actuator(mjm, nworld, 12, ctrl)
  (aadr, an, _, _, _), (sadr, sn, _, _, _) = _buffers(mjm)[("act", 0)], _buffers(mjm)[("sens", 0)]
  for i in range(12):
    for w in range(nworld):
      for adr, n in ((aadr, an), (sadr, sn)):
        lt = ht.Buffer.from_flat(hist[i, w], adr, n, 1).logical_times()
        want = times[max(0, i + 1 - n) : i + 1, w]  # the start times of the steps so far, nothing of the sub-evaluations
        np.testing.assert_array_equal(lt[n - len(want) :], want)
        assert (lt[: n - len(want)] < 0).all()
      assert ht.Buffer.from_flat(hist[i, w], aadr, an, 1).logical_values()[-1, 0] == ctrl[i, w, 0]
  # all four evaluations of a step run at the step's start time and are driven by what the first one read, before the step's sample went in
  np.testing.assert_array_equal(force[:, :, 0], _truth_actuator(mjm, times, ctrl, nworld))
  k = round(delay / 0.01)
  np.testing.assert_array_equal(force[k:, :, 0], ctrl[: 12 - k, :, 0])


def _step_sensors(mjm, nworld, nstep, before_step):
  m, d = mjw.put_model(mjm), mjw.make_data(mjm, nworld=nworld)
  sd, times = [], []
  for i in range(nstep):
    before_step(i, m, d)
    times.append(d.time.numpy().copy())
    mjw.step(m, d)
    sd.append(d.sensordata.numpy().copy())
  return np.array(sd), np.array(times), m, d


@pytest.mark.gpu
@pytest.mark.parametrize("delay,nsample,want", [(0.02, 3, [0, 0, 10, 20]), (0.04, 5, [0, 0, 0, 0, 10])])
def test_jointpos_delay(delay, nsample, want):
  mjm = mjcf.from_xml_string(slide_xml(sensors=f'<jointpos joint="j0" delay="{delay}" nsample="{nsample}"/>'))
  sd, _, _, _ = _step_sensors(mjm, 2, len(want), lambda i, m, d: d.qpos.fill_(10.0 * (i + 1)))
  assert sd[:, 0, 0].tolist() == want and sd[:, 1, 0].tolist() == want


def _check_twins(mjm, sd, times, pairs, nworld):
  """pairs: (fresh sensor, delayed sensor).  The delayed slice must be, bitwise, the protocol applied to the twin's readings (zero-order hold)."""
  bufs = _buffers(mjm)
  for fresh, delayed in pairs:
    adr, n, dim, interp, delay = bufs[("sens", delayed)]
    assert interp == ht.ZOH
    fa, da = int(mjm.sensor_adr[fresh]), int(mjm.sensor_adr[delayed])
    for w in range(nworld):
      buf = ht.Buffer.initial(n, dim, 0.0, np.float32(0.01))
      buf.times = buf.times.astype(np.float32).astype(np.float64)
      for i in range(len(sd)):
        want = ht.evaluate(buf, float(times[i][w]), delay, interp, sd[i, w, fa : fa + dim], True)
        np.testing.assert_array_equal(sd[i, w, da : da + dim], want, err_msg=f"sensor {delayed} world {w} step {i}")
    assert np.abs(sd[-1, :, da : da + dim]).max() > 0  # (the delay has passed: real readings are being compared)


@pytest.mark.gpu
@pytest.mark.parametrize("delay,nsample", [(0.01, 1), (0.02, 2)])
def test_vector_sensors_read_before_they_insert(delay, nsample):
  """nsample 1 and 2: the slot the fresh reading goes to is the slot the delayed reading comes from."""
  mjm = mjcf.from_xml_string(BALL_XML.format(d=delay, n=nsample))

  def spin(i, m, d):
    if i == 0:
      d.qvel.assign(np.array([[1.0, -2.0, 0.5], [0.3, 0.7, -1.1]], dtype=np.float32))

  sd, times, _, _ = _step_sensors(mjm, 2, 8, spin)
  _check_twins(mjm, sd, times, [(0, 2), (1, 3)], 2)


MIXED_ACT = '<motor name="a0" joint="j0" delay="0.02" nsample="2"/><motor name="a1" joint="j1" delay="0.03" nsample="4"/>'
MIXED_SENS = ('<jointpos joint="j0"/><jointvel joint="j1"/><actuatorfrc actuator="a1"/><accelerometer site="s1"/>'
              '<jointpos joint="j0" delay="0.03" nsample="3"/><accelerometer site="s1" delay="0.02" nsample="2"/>'
              '<jointvel joint="j1" delay="0.01" nsample="5"/><actuatorfrc actuator="a1" delay="0.02" nsample="4"/>')


@pytest.mark.gpu
def test_two_actuators_and_sensors_of_every_stage_with_their_own_delays():
  mjm = mjcf.from_xml_string(slide_xml(actuators=MIXED_ACT, sensors=MIXED_SENS, njoint=2))
  nworld, nstep = 2, 10
  ctrl = _ctrl_seq(nworld, nstep, nu=2)
  m, d = mjw.put_model(mjm), mjw.make_data(mjm, nworld=nworld)
  assert m.nsensor_history_posvel == 3 and m.nsensor_history_acc == 1
  sd, times, force = [], [], []
  for i in range(nstep):
    d.ctrl.assign(ctrl[i])
    times.append(d.time.numpy().copy())
    mjw.step(m, d)
    sd.append(d.sensordata.numpy().copy())
    force.append(d.actuator_force.numpy().copy())
  sd, force = np.array(sd), np.array(force)
  for u in range(2):
    np.testing.assert_array_equal(force[:, :, u], _truth_actuator(mjm, times, ctrl, nworld, u))
  _check_twins(mjm, sd, times, [(0, 4), (3, 5), (1, 6), (2, 7)], nworld)


def _bound(buf):
  return 32 * ULP32 * max(np.abs(buf.values).max(), 1e-30)


@pytest.mark.gpu
@pytest.mark.parametrize("interp", ["linear", "cubic"])
def test_interpolated_delay_between_samples(interp):
  mjm = mjcf.from_xml_string(slide_xml(actuators=f'<motor joint="j0" delay="0.025" nsample="5" interp="{interp}"/>'))
  adr, n, _, code, delay = _buffers(mjm)[("act", 0)]
  assert code == {"linear": ht.LINEAR, "cubic": ht.CUBIC}[interp]
  nworld, nstep = 2, 12
  ctrl = _ctrl_seq(nworld, nstep)
  m, d = mjw.put_model(mjm), mjw.make_data(mjm, nworld=nworld)
  worst = 0.0
  for i in range(nstep):
    d.ctrl.assign(ctrl[i])
    t, rows = d.time.numpy().copy(), d.history.numpy().copy()
    mjw.step(m, d)
    got = d.actuator_force.numpy()
    for w in range(nworld):
      buf = ht.Buffer.from_flat(rows[w], adr, n, 1)
      want = buf.read(float(np.float32(t[w] - np.float32(delay))), code)[0]
      err = abs(float(got[w, 0]) - want)
      worst = max(worst, err / _bound(buf))
      assert err <= _bound(buf), (i, w, got[w, 0], want)
  print(f"interp {interp}: worst error {worst:.3f} of the 32-ulp bound")
  assert np.abs(got).max() > 0


@pytest.mark.gpu
def test_zero_delay_records_history_and_applies_ctrl_at_once():
  mjm = mjcf.from_xml_string(slide_xml(actuators='<motor joint="j0" delay="0" nsample="3"/>'))
  nworld, ctrl = 2, _ctrl_seq(2, 6)
  force, times, hist, d = _run_actuator(mjm, nworld, 6, ctrl)
  np.testing.assert_array_equal(force, ctrl)
  m = mjw.put_model(mjm)
  res = mjw.DeviceArray.zeros((nworld,))
  for back in range(3):  # the three newest samples, by their own times
    mjw.read_ctrl(m, d, 0, mjw.DeviceArray.from_numpy(times[5 - back]), -1, res)
    np.testing.assert_array_equal(res.numpy(), ctrl[5 - back, :, 0])


def _warm(mjm, nworld, nstep):
  ctrl = _ctrl_seq(nworld, nstep, nu=max(mjm.nu, 1))
  m, d = mjw.put_model(mjm), mjw.make_data(mjm, nworld=nworld)
  for i in range(nstep):
    if mjm.nu:
      d.ctrl.assign(ctrl[i][:, : mjm.nu])
    d.qvel.assign(np.tile(np.float32(0.1 * (i + 1)), d.qvel.shape))
    mjw.step(m, d)
  return m, d


@pytest.mark.gpu
def test_read_ctrl_and_read_sensor_at_arbitrary_times():
  mjm = mjcf.from_xml_string(slide_xml(actuators='<motor joint="j0" delay="0.015" nsample="6" interp="cubic"/><motor joint="j0"/>',
                                       sensors='<jointvel joint="j0"/><framelinvel objtype="site" objname="s0" delay="0.02" nsample="5" interp="linear"/>'))
  nworld = 3
  m, d = _warm(mjm, nworld, 9)
  rows, now = d.history.numpy(), d.time.numpy()
  bufs = _buffers(mjm)
  q = np.array([[now[0] + 1.0, now[1] - 0.0237, now[2] - 0.05], [now[0] - 0.031, now[1] - 0.04, now[2]], [-5.0, now[1] - 0.0449, now[2] - 0.0012]], dtype=np.float32)
  for kind, i, read, shape in (("act", 0, mjw.read_ctrl, (nworld,)), ("sens", 1, mjw.read_sensor, (nworld, 3))):
    adr, n, dim, code, delay = bufs[(kind, i)]
    res = mjw.DeviceArray.zeros(shape)
    for interp in (-1, 0, 1, 2):
      for times in q:
        read(m, d, i, mjw.DeviceArray.from_numpy(times), interp, res)
        got = res.numpy().reshape(nworld, dim)
        for w in range(nworld):
          buf = ht.Buffer.from_flat(rows[w], adr, n, dim)
          want = buf.read(float(np.float32(times[w] - np.float32(delay))), code if interp < 0 else interp)
          if interp == 0:
            np.testing.assert_array_equal(got[w], want)
          else:
            assert np.abs(got[w] - want).max() <= _bound(buf), (kind, interp, w, got[w], want)
  # without a buffer: Data.ctrl / the sensor's slice of sensordata
  res = mjw.DeviceArray.zeros((nworld,))
  mjw.read_ctrl(m, d, 1, mjw.DeviceArray.from_numpy(q[0]), -1, res)
  np.testing.assert_array_equal(res.numpy(), d.ctrl.numpy()[:, 1])
  res = mjw.DeviceArray.zeros((nworld, 1))
  mjw.read_sensor(m, d, 0, mjw.DeviceArray.from_numpy(q[0]), 2, res)
  np.testing.assert_array_equal(res.numpy(), d.sensordata.numpy()[:, :1])


@pytest.mark.gpu
def test_init_history_and_an_insert_that_meets_an_existing_time():
  mjm = mjcf.from_xml_string(slide_xml(actuators='<motor joint="j0" delay="0.01" nsample="3"/>', sensors='<framepos objtype="site" objname="s0" delay="0.01" nsample="2"/>'))
  nworld = 2
  m, d = mjw.put_model(mjm), mjw.make_data(mjm, nworld=nworld)
  bufs = _buffers(mjm)
  (aadr, an, _, _, _), (sadr, sn, sdim, _, _) = bufs[("act", 0)], bufs[("sens", 0)]
  times = np.array([-0.02, -0.01, 0.0], dtype=np.float32)  # the newest sample sits at the time of the next step
  avals = np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]], dtype=np.float32)
  svals = np.arange(12, dtype=np.float32).reshape(2, 6) + 1
  phase = np.array([0.25, 0.5], dtype=np.float32)
  rows0 = d.history.numpy().copy()
  rows0[:, aadr] = 9.0  # the actuator's user slot survives its init
  d.history.assign(rows0)
  mjw.init_ctrl_history(m, d, 0, mjw.DeviceArray.from_numpy(times), mjw.DeviceArray.from_numpy(avals))
  mjw.init_sensor_history(m, d, 0, None, mjw.DeviceArray.from_numpy(svals), mjw.DeviceArray.from_numpy(phase))
  rows = d.history.numpy()
  for w in range(nworld):
    a, s = ht.Buffer.from_flat(rows[w], aadr, an, 1), ht.Buffer.from_flat(rows[w], sadr, sn, sdim)
    assert (a.user, a.cursor, s.user, s.cursor) == (9.0, an - 1, float(phase[w]), sn - 1)
    np.testing.assert_array_equal(a.times, times)
    np.testing.assert_array_equal(a.values[:, 0], avals[w])
    assert (s.times == np.float32(-1e10)).all()
    np.testing.assert_array_equal(s.values.ravel(), svals[w])
  # a step at t = 0: the actuator reads t - 0.01 (the middle sample), then its insert at t = 0 REPLACES the newest sample's value
  d.ctrl.assign(np.array([[7.0], [8.0]], dtype=np.float32))
  mjw.step(m, d)
  np.testing.assert_array_equal(d.actuator_force.numpy()[:, 0], avals[:, 1])
  after = d.history.numpy()
  for w in range(nworld):
    want = ht.Buffer.from_flat(rows[w], aadr, an, 1)
    want.insert(0.0, [7.0 + w])
    got = ht.Buffer.from_flat(after[w], aadr, an, 1)
    assert got.cursor == an - 1
    np.testing.assert_array_equal(got.flat(), want.flat())
    np.testing.assert_array_equal(got.values[:, 0], [avals[w, 0], avals[w, 1], 7.0 + w])


@pytest.mark.gpu
def test_a_buffer_that_wraps_many_times():
  mjm = mjcf.from_xml_string(slide_xml(actuators='<motor joint="j0" delay="0.02" nsample="3"/>'))
  ctrl = _ctrl_seq(2, 40)
  force, times, hist, _ = _run_actuator(mjm, 2, 40, ctrl)
  np.testing.assert_array_equal(force[:, :, 0], _truth_actuator(mjm, times, ctrl, 2))
  np.testing.assert_array_equal(force[2:, :, 0], ctrl[:38, :, 0])
  assert sorted(hist[-1, 0, 2:5].tolist()) == times[-3:, 0].tolist()


@pytest.mark.gpu
def test_get_state_set_state_replays_bitwise():
  mjm = mjcf.from_xml_string(slide_xml(actuators=MIXED_ACT, sensors=MIXED_SENS, njoint=2))
  nworld = 2
  ctrl = _ctrl_seq(nworld, 10, nu=2)
  m, d = mjw.put_model(mjm), mjw.make_data(mjm, nworld=nworld)

  def run(lo, hi):
    out = []
    for i in range(lo, hi):
      d.ctrl.assign(ctrl[i])
      mjw.step(m, d)
      out.append((d.actuator_force.numpy().copy(), d.sensordata.numpy().copy()))
    return out

  run(0, 5)
  state = mjw.DeviceArray.zeros((nworld, mjw.state_size(m, INTEGRATION)))
  mjw.get_state(m, d, state, INTEGRATION)
  first = run(5, 10)
  mjw.set_state(m, d, state, INTEGRATION)
  second = run(5, 10)
  for (f1, s1), (f2, s2) in zip(first, second):
    np.testing.assert_array_equal(f1, f2)
    np.testing.assert_array_equal(s1, s2)
  assert np.abs(first[-1][1]).max() > 0


@pytest.mark.gpu
def test_reset_data_with_a_mask_restores_only_those_worlds():
  mjm = mjcf.from_xml_string(slide_xml(actuators='<motor joint="j0" delay="0.02" nsample="3"/>', sensors='<jointvel joint="j0" delay="0.01" nsample="2"/>'))
  m, d = _warm(mjm, 3, 6)
  before, fresh = d.history.numpy().copy(), mjw.make_data(mjm, nworld=3).history.numpy()
  assert (before != fresh).any(axis=1).all()
  mjw.reset_data(m, d, np.array([True, False, True]))
  after = d.history.numpy()
  np.testing.assert_array_equal(after[[0, 2]], fresh[[0, 2]])
  np.testing.assert_array_equal(after[1], before[1])
  t = d.time.numpy()
  assert t[0] == 0.0 and t[2] == 0.0 and t[1] > 0.05


@pytest.mark.gpu
def test_runs_are_reproducible_and_independent_of_nworld():
  mjm = mjcf.from_xml_string(slide_xml(actuators=MIXED_ACT, sensors=MIXED_SENS, njoint=2))

  def run(nworld):
    ctrl = _ctrl_seq(nworld, 12, nu=2)
    m, d = mjw.put_model(mjm), mjw.make_data(mjm, nworld=nworld)
    out = []
    for i in range(12):
      d.ctrl.assign(ctrl[i])
      mjw.step(m, d)
      out.append(np.concatenate([d.actuator_force.numpy(), d.sensordata.numpy(), d.history.numpy()], axis=1))
    return np.array(out)

  a, b, one = run(5), run(5), run(1)
  np.testing.assert_array_equal(a, b)
  np.testing.assert_array_equal(a[:, :1], one)
