"""Constraint assembly (csrc/constraint.hpp make_constraint_body<G>) over row mixes, lane classes and njmax cuts: every case of
tests/constraint_models.py, 19 worlds in 19 different states -- so that ne / nf / nl / ncon and the active sets differ between the worlds of one
workgroup --, every world against its own float64 oracle run, integers exactly and floats row by row: through `forward` (k_mid<16|32|64>) and
through the stage API with the outputs poisoned first (k_make_constraint<32|64>).

One comparison function (`compare`) serves the GPU tests and the CPU twin test, which feeds it the float32 build of the oracle in place of
the device and divides every bound by 4: a case the float32 restatement of the algorithm cannot resolve to a quarter of a bound says nothing
about a kernel, and has to change, not the bound.

Checks per world
  exact         ne, nf, nl, nefc (counted in full past njmax), ncon, the NEFC overflow bit; efc.type; efc.id (contact rows: world-local contact);
                contact.dim; contact.efc_address with its -1 entries past njmax and past a contact's rows; J's pad columns are 0
  per row       rows < min(nefc, njmax) of J, D, aref, pos, vel, margin, frictionloss:
                max|d row| <= tol x max(max|oracle row|, floor x max|oracle field|), tol = test_gpu.py's SMOOTH (2e-5) for J and EFC (5e-4) for the
                rest; field = the world's rows of that array.  FLOOR per field, started at 1e-3 and raised only as far as the twin needs with
                its factor 4.  In brackets the smallest floor at which the twin's worst row -- over all cases and worlds -- meets bound / 4,
                and the case that sets it (0: every row meets the bound relative to itself):
                  J 1e-3 (0)   D 1e-3 (0)   aref 4.63e-3 (4.621e-3 rounded up to three digits, g16_act17; 1.7e-3 win_ncon32, 1.3e-3 win_hole)   pos 1e-3 (0)
                  vel 1e-3 (5.4e-4, g32_ncon33)   margin 1e-3 (0)   frictionloss 1e-3 (0)   Jqvel 1e-3 (1.4e-4, g64_ncon64)
                aref = -k imp pos - b vel: with the stiff parameter sets the two terms are hundreds of times the result of a row far below the
                field's maximum, which then carries the rounding of its terms.  D near an impedance clamp needed no floor above 1e-3.
                (Figures: profiles/constraint_sweep.txt; the tests print them again with -s.)
  own outputs   from the outputs under test alone, float64 on the host: J qvel = efc.vel per row within EFC relative to
                max(|vel|, floor x max|vel|) (floor "Jqvel": the one place where the kernel's recombined basis velocities meet its own J); the
                row pairs of a pyramidal contact all imply the same normal row, (J[2k] + J[2k+1]) / 2, within SMOOTH of its maximum; friction
                rows, scalar limit rows and single-joint equality rows have exactly one non-zero entry, and it is +-1
  cuts          njmax is placed by `sizes` from world 0's oracle rows; every world, the neighbours of an overflowing one included, is compared
                in full, so a row written across the per-world stride shows in the next world

The generator keeps every activation quantity (limit pos of every limited joint, dist - includemargin of every detected contact) at least 1e-3
from zero; the twin test asserts >= 1e-4 from the float64 oracle.

CPU pins of the oracle itself, over the same cases: finite differences (J v against the central difference of efc.pos along v, for equality,
limit, frictionless and elliptic normal rows) and `efc_row` restated in numpy from the definitions (D, aref, pos of every row at rtol 1e-12).
"""

import functools

import numpy as np
import pytest

import constraint_models as cm
import mujoco_warp_amd as mjw
import tree_models as tm
from mujoco_warp_amd import _npmath as nm
from mujoco_warp_amd import io
from oracle import ref
from test_gpu import EFC, SMOOTH

NWORLD = 19  # more than one workgroup at every worlds-per-workgroup count the launchers choose (1 .. 16), the last one partial: 19 is prime
ROWS = ("J", "D", "aref", "pos", "vel", "margin", "frictionloss")
FLOOR = dict(J=1e-3, D=1e-3, aref=4.63e-3, pos=1e-3, vel=1e-3, margin=1e-3, frictionloss=1e-3, Jqvel=1e-3)
INTS = ("ne", "nf", "nl", "nefc", "ncon", "overflow")
CT_EQUALITY, CT_FRICTION_DOF, CT_LIMIT_JOINT, CT_FRICTIONLESS, CT_PYRAMIDAL, CT_ELLIPTIC = 0, 1, 3, 5, 6, 7
ROOMY = 1536  # rows of the oracle runs that place the cuts and of the pins: no case comes near
MINVAL, MINIMP, MAXIMP = 1e-15, 1e-4, 0.9999
DSBL_REFSAFE = 1 << 12


@functools.lru_cache(maxsize=None)
def model(case):
  return mjw.mjcf.from_xml_string(cm.constraint_xml(case))


@functools.lru_cache(maxsize=None)
def states(case):
  return tuple(cm.world_state(case, model(case), w) for w in range(NWORLD))


def _record(s, njmax):
  """One world's rows and contacts from an oracle sim that has just run fwd_position (float64 copies)."""
  n, ncon = min(s.nefc, njmax), s.ncon
  rec = dict(ne=s.ne, nf=s.nf, nl=s.nl, nefc=s.nefc, ncon=ncon, overflow=bool(s.overflow & 1), type=s.efc_type[:n].copy(), id=s.efc_id[:n].copy(),
             dim=s.con_dim[:ncon].copy(), efc_address=s.con_efc_address[:ncon].copy(), qvel=np.array(s.qvel, dtype=np.float64), qpos=np.array(s.qpos, dtype=np.float64))
  for f in ROWS:
    rec[f] = np.array(getattr(s, "efc_" + f)[:n], dtype=np.float64)
  for f in ("dist", "includemargin", "solref", "solreffriction", "solimp", "friction", "geom"):  # (what the pins need)
    rec["con_" + f] = np.array(getattr(s, "con_" + f)[:ncon], dtype=np.float64 if f != "geom" else np.int32)
  return rec


class _Sim:
  """One oracle sim of a case that is put into the state of a world (eq_active included: the oracle reads it from its model struct)."""

  def __init__(self, case, real, nconmax, njmax):
    self.mjm, self.njmax = model(case), njmax
    self.s = ref.RefSim(self.mjm, nconmax=nconmax, njmax=njmax, real=real)
    self.eq = np.ctypeslib.as_array(self.s.cm.eq_active0, shape=(max(self.mjm.neq, 1),))

  def run(self, qpos, qvel, eq_active):
    s = self.s
    s.qpos[:], s.qvel[:] = qpos, qvel
    self.eq[: self.mjm.neq] = eq_active
    s.cd.overflow = 0
    s.stage("fwd_position")
    return _record(s, self.njmax)


@functools.lru_cache(maxsize=None)
def roomy_run(case):
  """Every world's float64 oracle record with room for every row and contact: what places the cut and what the pins read."""
  sim = _Sim(case, "f64", 96, ROOMY)
  out = tuple(sim.run(**st) for st in states(case))
  assert all(not r["overflow"] and r["ncon"] < 96 for r in out)
  return out


@functools.lru_cache(maxsize=None)
def sizes(case):
  """dict(njmax, nconmax) of a case.  Without a cut: room for every world's rows.  With one, njmax from the rows of world 0:
  exact = nefc | minus1 = nefc - 1 | eq = ne - 2 | fric = ne + nf - 2 | limit_ball = the row of the first ball limit (the first dropped row is a
  ball row) | ("con", a, k) = the first row of the a-th active contact + k | window_past = ("con", 14, 0): the budget ends with window 0 and the
  first active contact of window 1 is past it | an int."""
  mjm, cut, recs = model(case), cm.CASES[case]["cut"], roomy_run(case)
  r0 = recs[0]
  if cut == "window_past":
    cut = ("con", 14, 0)
  if cut is None:
    njmax = max(r["nefc"] for r in recs) + 5
  elif isinstance(cut, int):
    njmax = cut
  elif cut in ("exact", "minus1"):
    njmax = r0["nefc"] - (cut == "minus1")
  elif cut == "eq":
    njmax = r0["ne"] - 2
  elif cut == "fric":
    njmax = r0["ne"] + r0["nf"] - 2
  elif cut == "limit_ball":
    njmax = next(r for r in range(r0["nefc"]) if r0["type"][r] == CT_LIMIT_JOINT and mjm.jnt_type[r0["id"][r]] == 1)
  else:
    first = [int(a[0]) for a in r0["efc_address"] if a[0] >= 0]
    njmax = first[cut[1]] + cut[2]
  return dict(njmax=int(njmax), nconmax=max(max(r["ncon"] for r in recs) + 3, 8))


@functools.lru_cache(maxsize=None)
def oracle_run(case, real="f64"):
  """Every world's record at the case's njmax from the oracle (real="f32": the float32 twin).  Computed once per case and shared; callers do not
  write to it."""
  sz = sizes(case)
  sim = _Sim(case, real, sz["nconmax"], sz["njmax"])
  return tuple(sim.run(**st) for st in states(case))


def _rowmax(x):
  x = np.abs(x)
  return x.reshape(x.shape[0], -1).max(axis=1)


def compare(case, path, got, want, div=1.0):
  """(failures, figures): `got` (the device's records, or the twin's) against the oracle's `want`, one record per world, under the header's
  bounds divided by `div`.  A failure names case, path, world, field and row.  figures: per field the worst row as a fraction of its bound and
  the floor that row would need."""
  mjm, njmax = model(case), sizes(case)["njmax"]
  fails = []
  fig = {f: dict(row=0.0, floor=0.0) for f in FLOOR}
  fig["pyramid"] = 0.0

  def row_check(tag, name, g, o, tol):
    """rows of g against rows of o under the row bound; updates the figures of `name`."""
    if not np.isfinite(g).all():
      fails.append(f"{tag} {name}: not finite")
      return
    drow, orow = _rowmax(g - o), _rowmax(o)
    fmax = orow.max()
    bound = tol / div * np.maximum(orow, FLOOR[name] * fmax)
    with np.errstate(divide="ignore", invalid="ignore"):
      frac = np.where(drow > 0, drow / bound, 0.0)  # (a field that is zero throughout -- margin, world 7's velocities -- must be exactly so)
      need = np.where(drow > tol / div * orow, drow / (tol / div * fmax), 0.0)
    i = int(np.argmax(frac))
    fig[name]["row"] = max(fig[name]["row"], float(frac[i]))
    fig[name]["floor"] = max(fig[name]["floor"], float(need.max()))
    if frac[i] > 1:
      fails.append(f"{tag} {name} row {i}: |d| {drow[i]:.3e} > {bound[i]:.3e} (row max {orow[i]:.3e}, field max {fmax:.3e})")

  for w in range(NWORLD):
    g, o, tag = got[w], want[w], f"{case} {path} world {w}"
    bad = [f"{k} {g[k]} != {o[k]}" for k in INTS if g[k] != o[k]]
    n = min(o["nefc"], njmax)
    assert len(o["type"]) == n
    k = g["efc_address"].shape[1] if g["efc_address"].ndim == 2 else 10  # (the device keeps nmaxpyramid columns: the rest must be unused)
    if not (o["efc_address"][:, k:] == -1).all():
      bad.append(f"efc_address: the oracle uses more than {k} columns")
    for name, gi, oi in (("efc.type", g["type"], o["type"]), ("efc.id", g["id"], o["id"]), ("contact.dim", g["dim"], o["dim"]),
                         ("contact.efc_address", g["efc_address"], o["efc_address"][:, :k])):
      if not bad and (gi.shape != oi.shape or (gi != oi).any()):
        bad.append(f"{name}: {gi.tolist()} != {oi.tolist()}")
    if "Jpad" in g and not bad and not (g["Jpad"] == 0).all():
      bad.append("efc.J: non-zero pad columns")
    if bad:
      fails += [f"{tag} {b}" for b in bad[:3]]
      continue
    if n == 0:
      continue
    for f in ROWS:
      row_check(tag, f, g[f], o[f], SMOOTH if f == "J" else EFC)
    # from the outputs under test alone
    J, vel, typ = g["J"], g["vel"], o["type"]
    if np.isfinite(J).all() and np.isfinite(vel).all():
      row_check(tag, "Jqvel", J @ g["qvel"], vel, EFC)
      r = 0
      while r < n:
        if typ[r] != CT_PYRAMIDAL:
          if typ[r] in (CT_FRICTION_DOF, CT_LIMIT_JOINT, CT_EQUALITY):
            onehot = typ[r] == CT_FRICTION_DOF or (typ[r] == CT_LIMIT_JOINT and mjm.jnt_type[o["id"][r]] != 1) or (typ[r] == CT_EQUALITY and mjm.eq_obj2id[o["id"][r]] < 0)
            nz = J[r][J[r] != 0]
            if onehot and not (len(nz) == 1 and abs(nz[0]) == 1.0):
              fails.append(f"{tag} J row {r}: a one-hot row holds {nz.tolist()}")
          r += 1
          continue
        c = o["id"][r]
        rows = [x for x in o["efc_address"][c] if x >= 0]
        normals = [(J[a] + J[a + 1]) / 2 for a in rows[0::2] if a + 1 in rows]
        for nrm in normals[1:]:
          e = np.abs(nrm - normals[0]).max() / np.abs(normals[0]).max()
          fig["pyramid"] = max(fig["pyramid"], float(e))
          if e > SMOOTH / div:
            fails.append(f"{tag} contact {c}: the row pairs imply normal rows {e:.3e} apart (> {SMOOTH / div:.1e})")
        r = rows[-1] + 1
  return fails, fig


def summary(case, path, fig):
  rows = "  ".join(f"{f} {fig[f]['row']:.2f}/{fig[f]['floor']:.1e}" for f in FLOOR)
  sz = sizes(case)
  return f"{case:18s} {path:7s} njmax {sz['njmax']:4d} {rows}  pyramid normals {fig['pyramid']:.1e}"  # (per field: worst row as a fraction of its bound / floor needed)


# ---- numpy restatements for the pins ---------------------------------------------------------------------------------------------------


def efc_row_np(timestep, refsafe, pos_aref, pos_imp, invweight, solref, solimp, margin, vel):
  """(D, aref, pos) of one row from the definitions: stiffness k and damping b from solref (time constant and damping ratio, or direct when
  negative), the impedance curve of solimp at |pos_imp| / width, D = imp / (invweight (1 - imp))."""
  timeconst, dampratio = solref
  dmin, dmax, width, mid, power = solimp
  if refsafe:
    timeconst = max(timeconst, 2 * timestep)
  dmin, dmax, mid = (min(max(x, MINIMP), MAXIMP) for x in (dmin, dmax, mid))
  width, power = max(width, MINVAL), max(power, 1.0)
  k = 1 / (dmax * dmax * timeconst * timeconst * dampratio * dampratio) if solref[0] > 0 else -solref[0] / (dmax * dmax)
  b = 2 / (dmax * timeconst) if solref[1] > 0 else -solref[1] / dmax
  x = abs(pos_imp) / width
  if x > 1:  # past the width: full impedance
    imp = dmax
  else:
    y = x ** power / mid ** (power - 1) if x < mid else 1 - (1 - x) ** power / (1 - mid) ** (power - 1)
    imp = min(max(dmin + y * (dmax - dmin), dmin), dmax)
  return 1 / max(invweight * (1 - imp) / imp, MINVAL), -k * imp * pos_aref - b * vel, pos_aref + margin


def row_params(mjm, rec):
  """[(pos_aref, pos_imp, invweight, solref, solimp, margin)] of a record's rows, from the model and the record's contacts."""
  out = []
  iw_dof, iw_body, impratio = np.asarray(mjm.dof_invweight0), np.asarray(mjm.body_invweight0).reshape(-1, 2), float(mjm.opt.impratio)
  for r, (t, i) in enumerate(zip(rec["type"], rec["id"])):
    pos = rec["pos"][r]
    if t == CT_EQUALITY:
      j1, j2 = int(mjm.eq_obj1id[i]), int(mjm.eq_obj2id[i])
      iw = iw_dof[mjm.jnt_dofadr[j1]] + (iw_dof[mjm.jnt_dofadr[j2]] if j2 >= 0 else 0.0)
      out.append((pos, pos, iw, mjm.eq_solref[i], mjm.eq_solimp[i], 0.0))
    elif t == CT_FRICTION_DOF:
      out.append((0.0, 0.0, iw_dof[i], mjm.dof_solref[i], mjm.dof_solimp[i], 0.0))
    elif t == CT_LIMIT_JOINT:
      mg = float(mjm.jnt_margin[i])
      out.append((pos - mg, pos - mg, iw_dof[mjm.jnt_dofadr[i]], mjm.jnt_solref[i], mjm.jnt_solimp[i], mg))
    else:
      mg, fri, dim = rec["con_includemargin"][i], rec["con_friction"][i], int(rec["dim"][i])
      p = rec["con_dist"][i] - mg
      b1, b2 = (int(mjm.geom_bodyid[g]) for g in rec["con_geom"][i])
      iw, solref, pa = iw_body[b1, 0] + iw_body[b2, 0], rec["con_solref"][i], p
      if t == CT_PYRAMIDAL:
        iw = (iw + fri[0] * fri[0] * iw) * 2 * fri[0] * fri[0] / impratio
      elif t == CT_ELLIPTIC:
        dimid = r - int(rec["efc_address"][i][0])
        if dimid > 0:
          pa, iw = 0.0, iw / impratio
          if rec["con_solreffriction"][i].any():
            solref = rec["con_solreffriction"][i]
        if dimid > 1:
          iw *= fri[0] * fri[0] / (fri[dimid - 1] * fri[dimid - 1])
      out.append((pa, p, iw, solref, rec["con_solimp"][i], mg))
  return out


def integrate_pos(mjm, qpos, v, h):
  """qpos moved along the velocity v for the time h: quaternions of free and ball joints turn about their local axes (mujoco_warp_amd._npmath)."""
  q = np.array(qpos, dtype=np.float64)
  for j in range(mjm.njnt):
    t, a, d = int(mjm.jnt_type[j]), int(mjm.jnt_qposadr[j]), int(mjm.jnt_dofadr[j])
    if t == 0:
      q[a : a + 3] += h * v[d : d + 3]
      a, d = a + 3, d + 3
    if t in (0, 1):
      ang = np.linalg.norm(v[d : d + 3]) * h
      if ang != 0:
        q[a : a + 4] = nm.quat_normalize(nm.quat_mul(nm.quat_normalize(q[a : a + 4]), nm.axis_angle_to_quat(v[d : d + 3] / np.linalg.norm(v[d : d + 3]), ang)))
    else:
      q[a] += h * v[d]
  return q


CON_WINDOW, CON_STRIDE, LDS_PER_CU = 16, 32, 160 * 1024  # csrc/contact_rec.hpp, dev_common.hpp, host.hpp


def con_layout_words(nv, njmax, ncap, nbody, ngeom):
  """LDS words of one world in constraint assembly: con_layout of csrc/constraint.hpp, restated (cdof, qvel, three row tables, the active list,
  the window's staged records, subtree com, geom body, body root, the bodies' dof masks)."""
  o = 6 * nv + nv + 3 * njmax + 3 * ncap + CON_WINDOW * CON_STRIDE + 3 * nbody + ngeom + nbody + nbody * ((nv + 31) // 32)
  return (o + 3) // 4 * 4 + 1


def mid_worlds_per_workgroup(words, G):
  """Collision + constraint worlds per workgroup of k_mid<G> (launch_mid_g of csrc/mjhip.hip, restated): 256 / G, halved while they need more than
  half a CU's LDS.  `words` from con_layout alone is a lower bound of the kernel's stride, so the result is an upper bound."""
  nw = 256 // G
  while nw > 1 and 4 * words * nw > LDS_PER_CU // 2:
    nw >>= 1
  return nw


def activation(mjm, rec):
  """Every activation quantity of a world: pos of every limited joint (active or not) and dist - includemargin of every detected contact."""
  out = list(rec["con_dist"] - rec["con_includemargin"])
  for j in np.flatnonzero(mjm.jnt_limited):
    t, a, mg = int(mjm.jnt_type[j]), int(mjm.jnt_qposadr[j]), float(mjm.jnt_margin[j])
    if t == 1:
      q = nm.quat_normalize(rec["qpos"][a : a + 4])
      out.append(max(mjm.jnt_range[j]) - 2 * np.arctan2(np.linalg.norm(q[1:]), abs(q[0])) - mg)
    else:
      out.append(min(rec["qpos"][a] - mjm.jnt_range[j][0], mjm.jnt_range[j][1] - rec["qpos"][a]) - mg)
  return np.array(out)


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------------

ALL = list(cm.CASES)


@pytest.mark.parametrize("case", ALL)
def test_case_has_its_sizes_and_boundary(case):
  cfg, mjm, recs = cm.CASES[case], model(case), roomy_run(case)
  assert cm.constraint_xml(case) == cm.constraint_xml(case) == cm.constraint_xml(dict(cfg))  # deterministic
  assert (mjm.nbody, mjm.nv, mjm.njnt, mjm.ngeom) == cm.sizes_of(cfg)
  lanes = tm.lane_groups(mjm.nbody, mjm.nv)
  assert (lanes[2], 64 if lanes[1] == 64 else 32) == cfg["lanes"]  # (k_mid, k_make_constraint: 64 lanes where k_fwd_vel has them)
  assert not cfg["pair"] or (cfg["lanes"] == (32, 32) and mjm.npair == 1)  # (an explicit pair pins every kernel to 32 lanes: only where the sizes choose them anyway)
  assert set(int(t) for t in mjm.geom_type) <= {0, 2}  # planes and spheres: the light collision instantiation, which leaves the lane choice to the sizes
  full = [recs[w] for w in range(0, NWORLD, 3)]
  nact = lambda r: int((r["efc_address"][:, 0] >= 0).sum()) if r["ncon"] else 0
  name = case.split("_")[-1]
  for key, count in (("neq", lambda r: r["ne"]), ("nf", lambda r: r["nf"]), ("nl", lambda r: r["nl"]), ("ncon", lambda r: r["ncon"]), ("act", nact)):
    if name.startswith(key) and name[len(key):].isdigit():
      if key == "neq" and not cfg["eq_all"] and mjm.neq:  # (inactive ones interleaved: the count is the model's, the rows are fewer)
        assert mjm.neq == int(name[3:]) and all(r["ne"] < mjm.neq for r in full)
        continue
      assert {count(r) for r in full} == {int(name[len(key):])}, (case, [count(r) for r in full])
      assert len({count(r) for r in recs}) > 1 or key == "nf" or name[len(key):] == "0", (case, key)  # (friction loss is the model's: the same in every world)
  # the worlds of one workgroup differ
  assert len({tuple(r["qpos"]) for r in recs}) == NWORLD
  if cfg["rake"] and not case.endswith("ncon0"):
    assert len({(r["ncon"], nact(r)) for r in recs}) >= 3 and any(r["ncon"] > nact(r) for r in recs)
  if any(mjm.jnt_limited):
    assert len({r["nl"] for r in recs}) >= 2
  if mjm.neq and not cfg["eq_all"]:
    assert len({r["ne"] for r in recs}) >= 2
  sz, r0 = sizes(case), recs[0]
  assert sz["njmax"] >= 1
  if cfg["cut"] is not None and not isinstance(cfg["cut"], int):
    assert (r0["nefc"] > sz["njmax"]) == (cfg["cut"] != "exact") and r0["nefc"] >= sz["njmax"]
    assert sum(r["nefc"] > sz["njmax"] for r in recs) >= 3
    assert any(r["nefc"] <= sz["njmax"] for r in recs) or cfg["cut"] in ("eq", "fric", "limit_ball")  # (a cut in the contacts: worlds on both sides of it)
  if case == "g16_ncon17":
    assert r0["dim"][15] == 6 and r0["efc_address"][15][0] >= 0
  if case == "win_hole":
    assert (r0["efc_address"][16:32, 0] == -1).all() and (r0["efc_address"][32:36, 0] >= 0).all() and (r0["efc_address"][:3, 0] >= 0).all()
  if case == "g64_nl64_ball":
    assert mjm.njnt == 64 and mjm.jnt_type[63] == 1 and r0["nl"] == 64 and r0["id"][r0["ne"] + r0["nf"] + 63] == 63
  if case.endswith("window_past"):
    first = [int(a[0]) for a in r0["efc_address"] if a[0] >= 0]
    assert (r0["efc_address"][14:16, 0] == -1).all() and r0["efc_address"][16][0] == first[14] == sz["njmax"]
  if case.endswith("limit_ball"):
    assert r0["type"][sz["njmax"]] == CT_LIMIT_JOINT and mjm.jnt_type[r0["id"][sz["njmax"]]] == 1
  if "con2p" in case:
    c = [i for i, a in enumerate(r0["efc_address"]) if a[0] >= 0][2]
    assert r0["dim"][c] == 6 and r0["efc_address"][c][0] < sz["njmax"] < r0["efc_address"][c][0] + (6 if cfg["cone"] == "elliptic" else 10)
  if name in ("neq0", "nf0", "nl0", "ncon0"):  # an empty section with rows in front of it (but for the equalities, the first) and behind it
    sec = [(r0["ne"], r0["nf"], r0["nl"], nact(r0)) for r0 in full]
    k = ("neq0", "nf0", "nl0", "ncon0").index(name)
    assert all(s[k] == 0 and (k == 0 or max(s[:k]) > 0) and (k == 3 or max(s[k + 1:]) > 0) and sum(x > 0 for x in s) == 3 for s in sec), (case, sec)
  if case == "njmax1024":
    # the row tables of con_layout (3 njmax words) leave k_mid<16> room for fewer collision + constraint worlds per workgroup than its default of 16
    words = con_layout_words(mjm.nv, sz["njmax"], io.contact_cap(sz["nconmax"]), mjm.nbody, mjm.ngeom)
    assert mjm.nv == 6 and sz["njmax"] == 1024 and cfg["lanes"][0] == 16
    assert mid_worlds_per_workgroup(words, 16) <= 4 < 256 // 16
  if case == "g16_mix":  # (the same class at an ordinary njmax keeps the default, as far as con_layout goes)
    words = con_layout_words(mjm.nv, sz["njmax"], io.contact_cap(sz["nconmax"]), mjm.nbody, mjm.ngeom)
    assert mid_worlds_per_workgroup(words, 16) == 256 // 16


def test_parameter_sets_reach_every_row_kind_and_branch():
  """PSETS on equalities, dofs, joints and geoms; over all cases the rows take both signs of solref, powers 2 and 3, both sides of mid,
  imp_x > 1, and a time constant below 2 timestep with and without the refsafe clamp."""
  mjm = model("g64_mix")
  fl = np.asarray(mjm.dof_frictionloss) > 0
  for name, tab in (("eq", mjm.eq_solref), ("dof", np.asarray(mjm.dof_solref)[fl]), ("jnt", np.asarray(mjm.jnt_solref)[np.asarray(mjm.jnt_limited) > 0]),
                    ("geom", np.asarray(mjm.geom_solref)[1:11])):
    assert len({tuple(x) for x in np.asarray(tab)}) == len(cm.PSETS), name
  seen = set()
  for case in ("g16_mix", "g16_mix_ell", "g32_mix_ell", "g64_mix"):
    mjm = model(case)
    safe = not (int(mjm.opt.disableflags) & DSBL_REFSAFE)
    for rec in roomy_run(case):
      for (pa, pi, iw, solref, solimp, mg), t in zip(row_params(mjm, rec), rec["type"]):
        x, mid = abs(pi) / max(solimp[2], MINVAL), min(max(solimp[3], MINIMP), MAXIMP)
        kind = "contact" if t >= CT_FRICTIONLESS else int(t)
        seen |= {(kind, "solref+" if solref[0] > 0 else "solref-"), (kind, f"power{solimp[4]:g}"), (kind, "x<mid" if x < mid else "x>=mid")}
        if x > 1:
          seen.add((kind, "x>1"))
        if 0 < solref[0] < 2 * mjm.opt.timestep:
          seen.add((kind, "clamped" if safe else "unclamped"))
  for kind in (CT_EQUALITY, CT_FRICTION_DOF, CT_LIMIT_JOINT, "contact"):
    want = {"solref+", "solref-", "power2", "power3", "x<mid", "clamped", "unclamped"} | ({"x>=mid", "x>1"} if kind != CT_FRICTION_DOF else set())
    assert want <= {b for k, b in seen if k == kind}, (kind, sorted(b for k, b in seen if k == kind))


@pytest.mark.parametrize("case", ALL)
def test_oracle_rows_match_efc_row_from_the_definitions(case):
  mjm = model(case)
  ts, safe = float(mjm.opt.timestep), not (int(mjm.opt.disableflags) & DSBL_REFSAFE)
  for w, rec in enumerate(roomy_run(case)):
    for r, p in enumerate(row_params(mjm, rec)):
      want = efc_row_np(ts, safe, *p, rec["vel"][r])
      got = (rec["D"][r], rec["aref"][r], rec["pos"][r])
      np.testing.assert_allclose(got, want, rtol=1e-12, atol=0, err_msg=f"{case} world {w} row {r} (type {rec['type'][r]}, id {rec['id'][r]}): D, aref, pos")
      assert rec["margin"][r] == p[5]


@pytest.mark.parametrize("case", ALL)
def test_oracle_jacobian_matches_finite_differences_of_pos(case):
  """J v = d pos / dt along v for every row whose pos is a function of qpos: equality, limit (ball included), frictionless and elliptic normal
  rows.  Central differences in float64 with step 1e-6 (truncation ~1e-10 relative), bound 1e-6 x max|J row|; the active set must not change."""
  mjm, h = model(case), 1e-6
  sim = _Sim(case, "f64", 96, ROOMY)
  rng = np.random.default_rng(5)
  checked = 0
  for w, (st, rec) in enumerate(zip(states(case), roomy_run(case))):
    covered = [r for r in range(len(rec["type"])) if rec["type"][r] in (CT_EQUALITY, CT_LIMIT_JOINT, CT_FRICTIONLESS)
               or (rec["type"][r] == CT_ELLIPTIC and rec["efc_address"][rec["id"][r]][0] == r)]
    if not covered:
      continue
    for _ in range(3):
      v = rng.standard_normal(mjm.nv)
      side = [sim.run(integrate_pos(mjm, st["qpos"], v, s * h), st["qvel"], st["eq_active"]) for s in (1.0, -1.0)]
      for x in side:
        assert (x["type"] == rec["type"]).all() and (x["id"] == rec["id"]).all() and (x["efc_address"] == rec["efc_address"]).all(), f"{case} world {w}: the active set changed"
      fd = (side[0]["pos"] - side[1]["pos"]) / (2 * h)
      jv = rec["J"] @ v
      for r in covered:
        assert abs(jv[r] - fd[r]) <= 1e-6 * np.abs(rec["J"][r]).max(), f"{case} world {w} row {r} (type {rec['type'][r]}, id {rec['id'][r]}): J v {jv[r]:.9e}, d pos {fd[r]:.9e}"
        checked += 1
  assert checked > 0


@pytest.mark.parametrize("case", ALL)
def test_float32_twin_resolves_the_case_with_margin(case):
  """The GPU test's comparison with every bound divided by 4, on the float32 build of the oracle: what keeps the GPU test honest.  Also the
  activation gap, from the float64 oracle: no limit or contact of any world is closer than 1e-4 to changing its state."""
  mjm, want = model(case), oracle_run(case)
  for w, rec in enumerate(roomy_run(case)):
    gap = np.abs(activation(mjm, rec))
    assert gap.size == 0 or gap.min() >= 1e-4, f"{case} world {w}: an activation quantity is {gap.min():.2e} from zero"
  fails, fig = compare(case, "twin", oracle_run(case, "f32"), want, div=4.0)
  print(summary(case, "twin", fig))
  assert not fails, "\n".join(fails[:20])


def test_compare_sees_a_wrong_small_row_and_a_shifted_row():
  """`compare` itself: the float64 oracle against itself passes with zero figures; one small row scaled by 1 + 1e-2 next to large ones, a row
  written one slot late, and a dropped -1 in efc_address each fail."""
  case = "g16_mix"
  want = oracle_run(case)
  fails, fig = compare(case, "self", want, want)
  assert not fails and max(fig[f]["row"] for f in ROWS) == 0 and fig["Jqvel"]["row"] < 1e-6  # (J qvel in another order of summation: rounding)
  w = 3

  def mutated(fn):
    rec = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in want[w].items()}
    fn(rec)
    return compare(case, "mutant", want[:w] + (rec,) + want[w + 1 :], want)[0]

  small = int(np.argmin(np.where(want[w]["D"] > 0, want[w]["D"], np.inf)))
  assert want[w]["D"][small] < 0.05 * want[w]["D"].max()

  def scale(rec):
    rec["D"][small] *= 1.01

  def shift(rec):
    rec["aref"][1:] = rec["aref"][:-1].copy()

  def address(rec):
    rec["efc_address"][0][0] = -1

  for fn, word in ((scale, f"D row {small}"), (shift, "aref row"), (address, "contact.efc_address")):
    out = mutated(fn)
    assert out and word in out[0], (word, out[:2])


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------

POISON = -7


def _device(case):
  mjm, st, sz = model(case), states(case), sizes(case)
  m = mjw.put_model(mjm)
  d = mjw.make_data(mjm, nworld=NWORLD, nconmax=sz["nconmax"], njmax=sz["njmax"])
  d.qpos.assign(np.array([s["qpos"] for s in st], dtype=np.float32))
  d.qvel.assign(np.array([s["qvel"] for s in st], dtype=np.float32))
  if mjm.neq:
    d.eq_active.assign(np.array([s["eq_active"] for s in st], dtype=np.int32))
  return mjm, m, d


def _fetch(mjm, d):
  """The device's records, one per world (efc.id of contact rows made world-local with ws_conadr)."""
  nv, njmax = mjm.nv, d.njmax
  cnt = {k: getattr(d, k).numpy() for k in ("ne", "nf", "nl", "nefc", "ws_ncon", "ws_conadr", "overflow")}
  efc = {f: getattr(d.efc, f).numpy() for f in ROWS + ("type", "id")}
  dim, adr_tab, qvel = d.contact.dim.numpy(), d.contact.efc_address.numpy(), d.qvel.numpy()
  out = []
  for w in range(NWORLD):
    n, ncon, adr = max(min(int(cnt["nefc"][w]), njmax), 0), int(cnt["ws_ncon"][w]), int(cnt["ws_conadr"][w])
    typ = efc["type"][w, :n]
    rec = dict(ne=int(cnt["ne"][w]), nf=int(cnt["nf"][w]), nl=int(cnt["nl"][w]), nefc=int(cnt["nefc"][w]), ncon=ncon,
               overflow=bool(int(cnt["overflow"][w]) & int(mjw.OverflowType.NEFC)), type=typ, id=efc["id"][w, :n] - adr * (typ >= CT_FRICTIONLESS),
               dim=dim[adr : adr + ncon], efc_address=adr_tab[adr : adr + ncon], qvel=qvel[w].astype(np.float64),
               J=efc["J"][w, :n, :nv].astype(np.float64), Jpad=efc["J"][w, :n, nv:])
    for f in ROWS[1:]:
      rec[f] = efc[f][w, :n].astype(np.float64)
    out.append(rec)
  return out


def _check(case, path, mjm, d):
  fails, fig = compare(case, path, _fetch(mjm, d), oracle_run(case))
  print(summary(case, path, fig))
  assert not fails, "\n".join(fails[:20])


@pytest.mark.gpu
@pytest.mark.parametrize("case", ALL)
def test_forward_matches_oracle_in_every_world(case):
  """The product path: `forward` (collision and constraint assembly inside k_mid at the case's lane count)."""
  mjm, m, d = _device(case)
  assert bool(m.heavy_colliders) == cm.CASES[case]["pair"] and not m.has_connect  # (an explicit pair: the heavy instantiation, 32 lanes whatever the sizes)
  mjw.forward(m, d)
  _check(case, "forward", mjm, d)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ALL)
def test_stage_api_matches_oracle_in_every_world(case):
  """The stage API: kinematics ... collision, make_constraint (k_make_constraint<32|64>), every output of the last two poisoned first."""
  mjm, m, d = _device(case)
  for fn in (mjw.kinematics, mjw.com_pos, mjw.crb, mjw.factor_m, mjw.com_vel):
    fn(m, d)
  for f in ROWS:
    getattr(d.efc, f).fill_(float("nan"))
  for a in (d.efc.type, d.efc.id, d.ne, d.nf, d.nl, d.nefc, d.contact.dim, d.contact.efc_address):
    a.fill_(POISON)
  mjw.collision(m, d)
  mjw.make_constraint(m, d)
  _check(case, "stages", mjm, d)
