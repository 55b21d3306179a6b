"""Host <-> device IO: the drop-in boundary of the engine.

Mirrors the reference's mujoco_warp/_src/io.py: put_model 259 (validation 284-360, derived tables 495-652),
make_data 1680, put_data 1890, get_data_into 2184, reset_data 2435, reset_data_keyframe 2797,
override_model 2933; default sizing _default_nconmax 1284 / _default_njmax 1299 / _get_padded_sizes 1268.
Same signatures, shapes, dtypes and error behaviour (ValueError / NotImplementedError at put/make time;
capacity problems at run time are bits in `d.overflow`).

Shapes and dtypes are stated once, in types.py (types.array_fields); the header says which of the arrays the library reads.  put_model
runs named phases (_check_supported, _tree_tables, _collision_facts, _actuator_facts, _options), each returning the sizes and host arrays
it derives; every other MjhModel array is the host model's attribute of that name, cast and reshaped to its declaration (_host_array,
_OPTIONAL_FIELDS for what a host model may lack).  make_data / put_data allocate every MjhData array from its declaration in the sizes of
_data_sizes.
"""

import ctypes
from typing import Optional

import numpy as np

from . import _abi
from . import trn_tables as transmission
from . import types
from .device import DeviceArray

from .mjcf import SENS as mjcf_SENS  # mjtSensor values of the supported sensors
from .mjcf import history_buffers, history_layout, history_row

_BATCHED_MODEL_FIELDS = [n[:-3] for n, k, p in _abi.MODEL_FIELDS if n.endswith("_nb")]
_MODEL_PTR_FIELDS = [n for n, k, p in _abi.MODEL_FIELDS if p]
_DATA_PTR_FIELDS = [n for n, k, p in _abi.DATA_FIELDS if p]


def _declared(*prefixed):
  """{ABI name: (shape, dtype, host)} of the arrays the given (prefix, class) pairs declare."""
  return {prefix + name: decl for prefix, cls in prefixed for name, decl in types.array_fields(cls).items()}


_MODEL_ARRAYS = _declared(("opt_", types.Option), ("stat_", types.Statistic), ("", types.Model))
_DATA_ARRAYS = _declared(("contact_", types.Contact), ("efc_", types.Constraint), ("", types.Data))


def _valid_sizes():
  return (2 + (np.arange(19) % 2)) * (2 ** (np.arange(19) // 2 + 3))


def _default_nconmax(mjm, mjd=None):
  vs = _valid_sizes()
  nconmax = max(45, getattr(mjd, "ncon", 0) if mjd is not None else 0)
  return int(nconmax) if nconmax > vs[-1] else int(vs[np.searchsorted(vs, nconmax)])


def _default_njmax(mjm, mjd=None):
  vs = _valid_sizes()
  njmax = max(53, getattr(mjd, "nefc", 0) if mjd is not None else 0)
  return int(njmax) if njmax > vs[-1] else int(vs[np.searchsorted(vs, njmax)])


def _get_padded_sizes(nv, njmax):
  def round_up(x, mult):
    return ((x + mult - 1) // mult) * mult

  return round_up(max(njmax, 1), 16), max(round_up(nv, 4), 4)


def is_sparse(mjm):
  jac = int(mjm.opt.jacobian)
  if jac == 2:  # auto
    return mjm.nv > 32
  return jac == 1


def geom_pairs(mjm):
  """Pre-filtered geom pairs in upper-triangular order (reference io.py:551-577, 631-640)."""
  filterparent = not (int(mjm.opt.disableflags) & types.DisableBit.FILTERPARENT)
  ng = mjm.ngeom
  if ng < 2:
    return np.zeros((0, 2), dtype=np.int32)
  g1, g2 = np.triu_indices(ng, k=1)
  b1, b2 = mjm.geom_bodyid[g1], mjm.geom_bodyid[g2]
  w1, w2 = mjm.body_weldid[b1], mjm.body_weldid[b2]
  wp1 = mjm.body_weldid[mjm.body_parentid[w1]]
  wp2 = mjm.body_weldid[mjm.body_parentid[w2]]
  self_col = w1 == w2
  parent_child = filterparent & (w1 != 0) & (w2 != 0) & ((w1 == wp2) | (w2 == wp1))
  mask = ((mjm.geom_contype[g1] & mjm.geom_conaffinity[g2]) | (mjm.geom_contype[g2] & mjm.geom_conaffinity[g1])) != 0
  exclude = np.isin((b1.astype(np.int64) << 16) + b2, np.asarray(mjm.exclude_signature, dtype=np.int64))
  keep = mask & ~self_col & ~parent_child & ~exclude
  return np.stack([g1[keep], g2[keep]], axis=1).astype(np.int32)


def geom_pairs_with_ids(mjm):
  """(pairs, pairid): the filtered pairs plus the explicit <contact><pair> entries, still in upper-triangular order; pairid is
  the explicit pair's index (its parameters override the geom mixing and it is included whatever the filters say) or -1
  (reference io.py:575-590 nxn_pairid)."""
  pairs = geom_pairs(mjm)
  npair = int(getattr(mjm, "npair", 0))
  if not npair:
    return pairs, np.full(len(pairs), -1, dtype=np.int32)
  table = {(int(a), int(b)): -1 for a, b in pairs}
  for i in range(npair):
    a, b = int(mjm.pair_geom1[i]), int(mjm.pair_geom2[i])
    table[(min(a, b), max(a, b))] = i
  keys = sorted(table)
  return np.array(keys, dtype=np.int32).reshape(-1, 2), np.array([table[k] for k in keys], dtype=np.int32)


_SUPPORTED_PAIRS = {(0, 2), (0, 3), (0, 4), (0, 5), (0, 6), (2, 2), (2, 3), (2, 5), (2, 6), (3, 3), (3, 6), (6, 6)}
# pairs of the reference's CONVEX class (collision_driver.py:47-80) that go through GJK / EPA (csrc/convex.hpp); box-box joins them
# unless DisableBit.NATIVECCD is set (collision_driver.py:867-870), see put_model
_CONVEX_PAIRS = {(2, 4), (3, 4), (3, 5), (4, 4), (4, 5), (4, 6), (5, 5), (5, 6), (2, 7), (3, 7), (4, 7), (5, 7), (6, 7), (7, 7)}
_HFIELD_PAIRS = {(1, 2), (1, 3), (1, 4), (1, 5), (1, 6), (1, 7)}  # height field vs convex geom: prism-wise GJK / EPA (collision_convex.py:164), heavy instantiation
_PLANE_MESH = (0, 7)  # primitive collider plane_convex (collision_primitive.py:52), heavy instantiation


def _pair_index(ngeom, pairs):
  """[ngeom (ngeom - 1) / 2] index into the filtered pair list of every unordered geom pair, -1 if filtered out (the SAP sweep's
  lookup; enumeration = math.upper_tri_index, reference math.py:323, collision_driver.py:485)."""
  out = np.full(max(ngeom * (ngeom - 1) // 2, 1), -1, dtype=np.int32)
  for p, (a, b) in enumerate(pairs):
    a, b = int(min(a, b)), int(max(a, b))
    out[(a * (2 * ngeom - a - 3)) // 2 + b - 1] = p
  return out


def _arr(x, dtype):
  return np.ascontiguousarray(np.asarray(x), dtype=dtype)


def cull_tables(geom_bodyid, pairs, pairid, geom_pos=None, geom_rbound=None):
  """Tables of k_broad_mask's group pre-test (csrc/collide.hpp): the pair list regrouped by PAIRS OF GEOM GROUPS, so that a world tests one
  bounding sphere per group pair before the bounding spheres of its geom pairs (the reference tests every geom pair, collision_driver.py:
  278-334; the pre-test only skips pairs whose sphere test must fail, the mask it produces is the same).

  A group is a maximal run of consecutive geoms of one moving body; every geom of the world body (static scenery spreads over the whole
  scene) is a group of its own; a group's sphere encloses its COLLIDING geoms only (the geoms of some non-explicit pair -- visual geoms have
  no bounding radius) and is centred on one of them, the CENTRE GEOM (the one that gives the smallest sphere in the body frame; any choice
  is valid, the kernel measures the radius in every world).  Returns
    cull_geom  [ncullgeom, 2]  geom + (group << 16) | the group's centre geom -- the colliding geoms, group by group
    cull_group [ncullgroup, 2] centre geom | number of colliding geoms (host-side description, not read by the kernel)
    cull_pair  [ncullpair, 4]  group | group | centre geom 1 + (centre geom 2 << 16) | first entry of cull_list + (count << 24), count <= 16
                               (longer group pairs are split into several rows); group -1: explicit pairs, whose margins are their own,
                               always tested
    cull_list  [npair, 2]      pair index | g1 + (g2 << 16)."""
  geom_bodyid = np.asarray(geom_bodyid).astype(np.int64)
  ng = len(geom_bodyid)
  i32 = np.int32
  if ng == 0 or len(pairs) == 0 or ng > 65535 or len(pairs) >= (1 << 24):
    return np.zeros((0, 2), i32), np.zeros((0, 2), i32), np.zeros((0, 4), i32), np.zeros((0, 2), i32)
  pairid = np.asarray(pairid)
  new = np.ones(ng, dtype=bool)
  new[1:] = (geom_bodyid[1:] != geom_bodyid[:-1]) | (geom_bodyid[1:] == 0)
  run = np.cumsum(new) - 1  # run of every geom
  used = np.zeros(ng, dtype=bool)
  used[pairs[pairid < 0].ravel()] = True
  geoms = np.flatnonzero(used)
  runs, first, count = np.unique(run[geoms], return_index=True, return_counts=True)  # (geoms ascending: a run's geoms are consecutive entries)
  gid = np.full(run.max() + 1, -1, dtype=np.int64)
  gid[runs] = np.arange(len(runs))
  centre = np.zeros(len(runs), dtype=np.int64)
  for k, (a, n) in enumerate(zip(first, count)):
    gs = geoms[a: a + n]
    centre[k] = gs[0]
    if n > 1 and geom_pos is not None and geom_rbound is not None:
      x, rb = np.asarray(geom_pos, dtype=np.float64).reshape(-1, 3)[gs], np.asarray(geom_rbound, dtype=np.float64).reshape(-1)[gs]
      radius = (np.linalg.norm(x[:, None, :] - x[None, :, :], axis=2) + rb[None, :]).max(axis=1)
      centre[k] = gs[int(np.argmin(radius))]
  cgeom = np.stack([geoms + (gid[run[geoms]] << 16), centre[gid[run[geoms]]]], axis=1)
  g1, g2 = pairs[:, 0].astype(np.int64), pairs[:, 1].astype(np.int64)
  key = gid[run[g1]] * (len(runs) + 1) + gid[run[g2]]
  key[pairid >= 0] = -1
  order = np.argsort(key, kind="stable")
  ks = key[order]
  start = np.flatnonzero(np.append(True, ks[1:] != ks[:-1]))
  cnt = np.diff(np.append(start, len(ks)))
  # (at most 16 entries per row: a quarter wavefront serves a surviving row, long group pairs are split)
  nchunk = (cnt + 15) // 16
  rows = np.repeat(np.arange(len(cnt)), nchunk)
  within = np.arange(len(rows)) - np.repeat(np.cumsum(nchunk) - nchunk, nchunk)
  ka, start, cnt = ks[start][rows], start[rows] + 16 * within, np.minimum(16, cnt[rows] - 16 * within)
  ga, gb = np.where(ka < 0, -1, ka // (len(runs) + 1)), np.where(ka < 0, -1, ka % (len(runs) + 1))
  cen = np.append(centre, 0)  # (rows of explicit pairs, group -1, have no centre geoms: the padding entry)
  cp = np.stack([ga, gb, np.where(ka < 0, 0, cen[ga] + (cen[gb] << 16)), start + (cnt << 24)], axis=1)
  cl = np.stack([order, g1[order] + (g2[order] << 16)], axis=1)
  return cgeom.astype(i32), np.stack([centre, count], axis=1).astype(i32), cp.astype(i32), cl.astype(i32)


def _condims(mjm, pairs):
  """condim values of the colliding geoms and of the explicit pairs."""
  condims = set(int(c) for c in np.unique(np.asarray(mjm.geom_condim)[np.unique(pairs)])) if len(pairs) else set()
  if int(getattr(mjm, "npair", 0)):
    condims |= set(int(c) for c in np.asarray(mjm.pair_dim))
  return condims


def _pair_types(mjm, pairs):
  """(smaller, larger) geom type of every pair."""
  gt = np.asarray(mjm.geom_type)
  return [(int(min(gt[a], gt[b])), int(max(gt[a], gt[b]))) for a, b in pairs]


def _check_supported(mjm, pairs):
  """Refuses what this engine does not compute (reference io.py:284-360): physics must not be dropped silently."""
  opt = mjm.opt
  if int(getattr(mjm, "neq", 0)) > 0:
    # connect and joint equalities are built (csrc/constraint.hpp); weld, tendon and flex are refused, and so is a connect with sleeping
    # enabled (csrc/sleep.hpp wakes and groups trees through the joints of an equality)
    names = getattr(mjm, "eq_names", None)
    who = lambda e: f"equality {e}" + (f" {names[e]!r}" if names is not None and len(names) > e and names[e] else "")
    for e, t in enumerate(np.asarray(mjm.eq_type).reshape(-1)):
      if int(t) not in (types.EqType.CONNECT, types.EqType.JOINT):
        kind = types.EqType(int(t)).name.lower() if int(t) in tuple(types.EqType) else f"type {int(t)}"
        raise NotImplementedError(f"{who(e)}: {kind} equality constraints are not implemented (connect and joint are)")
      if int(t) == types.EqType.CONNECT and (int(opt.enableflags) & int(types.EnableBit.SLEEP)):
        raise NotImplementedError(f"{who(e)}: a connect equality with sleeping enabled (EnableBit.SLEEP) is not implemented")
  for name in ("ntendon", "nflex", "nplugin"):
    if int(getattr(mjm, name, 0)) > 0:
      raise NotImplementedError(f"{name} > 0 is outside the hot-path scope of this engine")
  if int(opt.integrator) not in (types.IntegratorType.EULER, types.IntegratorType.RK4, types.IntegratorType.IMPLICITFAST, types.IntegratorType.IMPLICIT):
    raise NotImplementedError(f"Integrator {int(opt.integrator)} is unsupported.")
  if int(opt.integrator) == types.IntegratorType.IMPLICIT and mjm.nv > 64:
    raise NotImplementedError("The fully implicit integrator is implemented for models of at most 64 dofs (csrc/implicit.hpp); use implicitfast.")
  # (the reference rejects PGS, io.py solver check / types.py:502; this engine implements MuJoCo C's dual PGS, csrc/pgs.hpp)
  if int(opt.solver) not in (types.SolverType.PGS, types.SolverType.CG, types.SolverType.NEWTON):
    raise NotImplementedError(f"Unknown solver {int(opt.solver)}.")
  if int(opt.cone) not in (types.ConeType.PYRAMIDAL, types.ConeType.ELLIPTIC):
    raise NotImplementedError(f"Unknown cone {int(opt.cone)}.")
  if mjm.nu:
    transmission.check_types(mjm.actuator_trntype)  # (joint, jointinparent and site; body / slider-crank / tendon are refused by name)
    if not mjm.nv:
      raise NotImplementedError("actuators on a model without degrees of freedom are not implemented.")
  if int(getattr(opt, "noslip_iterations", 0)) > 0:
    raise NotImplementedError("noslip solver is unsupported.")
  if mjm.nu:
    for name, allowed, what in (("actuator_dyntype", (0, 1, 2, 3), "none / integrator / filter / filterexact"),
                                ("actuator_gaintype", (0, 1), "fixed / affine"), ("actuator_biastype", (0, 1), "none / affine")):
      if not np.isin(np.asarray(getattr(mjm, name)), allowed).all():
        raise NotImplementedError(f"{name}: only {what} are implemented (no muscle / user types).")
    if np.asarray(getattr(mjm, "actuator_actearly", [0])).any():
      raise NotImplementedError("actuator actearly is not implemented.")
    if (np.asarray(getattr(mjm, "actuator_actnum", [0])) > 1).any():
      raise NotImplementedError("actuators with more than one activation variable are not implemented.")
  for name in ("jnt_stiffnesspoly", "dof_dampingpoly"):
    if np.asarray(getattr(mjm, name, [0.0])).any():
      raise NotImplementedError(f"{name} (polynomial stiffness / damping) is not implemented.")
  if float(getattr(opt, "density", 0.0)) != 0.0 or float(getattr(opt, "viscosity", 0.0)) != 0.0:
    raise NotImplementedError("fluid forces (option density / viscosity, passive.py _fluid_force) are not implemented.")
  unsupported_enable = int(opt.enableflags) & int(types.EnableBit.OVERRIDE | types.EnableBit.FWDINV)
  if unsupported_enable:
    raise NotImplementedError(f"enable flags {types.EnableBit(unsupported_enable)!r} are not implemented.")
  # sleeping (reference io.py:356-360): Newton only; active when islands are not disabled (forward.py:345)
  if (int(opt.enableflags) & int(types.EnableBit.SLEEP)) and int(opt.solver) != int(types.SolverType.NEWTON):
    raise ValueError(f"sleeping requires the Newton solver (got solver={types.SolverType(int(opt.solver)).name})")
  if (int(opt.enableflags) & int(types.EnableBit.SLEEP)) and int(opt.integrator) == int(types.IntegratorType.RK4):
    raise NotImplementedError("sleeping with the RK4 integrator is not implemented.")
  gt = np.asarray(mjm.geom_type)
  for (a, b), t in zip(pairs, _pair_types(mjm, pairs)):
    if t in ((0, 1), (1, 1)):
      continue  # (plane / height-field against a height field: no collider in the reference either, collision_driver.py:47-59)
    if t not in _SUPPORTED_PAIRS and t not in _CONVEX_PAIRS and t != _PLANE_MESH and t not in _HFIELD_PAIRS:
      raise NotImplementedError(f"collision between geom types {t} is not implemented yet")
    if 7 in t:  # convex meshes: exhaustive vertex search, single contact
      for g in (a, b):
        if int(gt[g]) != 7:
          continue
        mid = int(np.asarray(getattr(mjm, "geom_dataid", np.full(len(gt), -1)))[g])
        if mid < 0 or not hasattr(mjm, "mesh_vert"):
          raise NotImplementedError("colliding mesh geom without mesh vertices (Model.mesh_vert / geom_dataid)")
  condims = _condims(mjm, pairs)
  if not condims <= {1, 3, 4, 6}:
    raise NotImplementedError(f"unsupported condim values {condims}")


def _collision_facts(mjm, pairs, pairid):
  """(sizes and flags, host arrays) of the collision pipeline: which kernel instantiation the model's pairs need, the buffers of the convex
  narrowphase, the pair tables."""
  opt, ngeom, nexplicit = mjm.opt, int(mjm.ngeom), int(getattr(mjm, "npair", 0))
  ptypes = _pair_types(mjm, pairs)
  # box-box is a CONVEX pair (GJK / EPA + multi-contact) unless DisableBit.NATIVECCD selects the primitive collider
  # (reference collision_driver.py:78, 867-870)
  box_ccd = not (int(opt.disableflags) & int(types.DisableBit.NATIVECCD))
  nboxbox = sum(t == (6, 6) for t in ptypes) if box_ccd else 0
  nconvex = sum(t in _CONVEX_PAIRS or t in _HFIELD_PAIRS for t in ptypes)
  convex_pairs = int(nconvex + nboxbox > 0)
  # capsule-box / box-box pairs and explicit contact pairs select the kernel instantiation that carries them (include/mjhip.h)
  heavy = int(any(t in ((3, 6), (6, 6), (0, 7)) for t in ptypes) or nexplicit > 0 or convex_pairs)
  # EPA iteration cap (reference collision_convex.py:1223): 16 when every convex pair of the model is box-box
  epa_iterations = 16 if (nboxbox > 0 and nconvex == 0) else int(getattr(opt, "ccd_iterations", 35))
  # clip buffers of the multi-contact recovery: 2 * npolygonmax points (reference collision_convex.py:1226-1234)
  nboxmesh, nmeshmesh = sum(t == (6, 7) for t in ptypes), sum(t == (7, 7) for t in ptypes)
  npolygonmax, nmeshdegmax = 4 if nboxbox > 0 else 0, 0
  if not (int(opt.disableflags) & int(types.DisableBit.MULTICCD)) and nboxmesh + nmeshmesh > 0:
    polyvertnum, polymapnum = np.asarray(getattr(mjm, "mesh_polyvertnum", ())), np.asarray(getattr(mjm, "mesh_polymapnum", ()))
    npolygonmax = max(int(polyvertnum.max()) if polyvertnum.size else 0, 4 if nboxmesh else npolygonmax)
    # polygons around one vertex (collision_convex.py:1233 nmeshdegmax): sizes the normal / index buffers of the multi-contact recovery
    nmeshdegmax = max(int(polymapnum.max()) if polymapnum.size else 0, 3)
  condims = _condims(mjm, pairs)
  nmaxcondim = int(max(condims)) if condims else 1
  # condim of every contact the model can make (collision_core.py contact_params: the geom of higher priority decides, the larger condim
  # at equal priority; explicit pairs carry their own): only 1 and 3 -> CG may run the contact-basis kernel (csrc/solver_cgp.hpp)
  gc_, gp_ = np.asarray(mjm.geom_condim).astype(int), np.asarray(mjm.geom_priority).astype(int)
  pair_condims = set(int(gc_[a] if gp_[a] > gp_[b] else gc_[b] if gp_[b] > gp_[a] else max(gc_[a], gc_[b])) for a, b in pairs)
  if nexplicit:
    pair_condims |= set(int(c) for c in np.asarray(mjm.pair_dim))
  # ... and no friction-loss rows (their three-zone cost is outside that kernel: it would hand EVERY world to its fallback launch, which
  # solves flagged worlds one after the other -- ADVICE round 5); the kernel still defers a world that shows up with nf > 0 (a model whose
  # frictionloss was edited after put_model), so this flag is about speed, not correctness
  has_floss = bool(np.any(np.asarray(getattr(mjm, "dof_frictionloss", 0.0)) > 0)) or bool(np.any(np.asarray(getattr(mjm, "tendon_frictionloss", 0.0)) > 0))
  cull = cull_tables(mjm.geom_bodyid, pairs, pairid, mjm.geom_pos, mjm.geom_rbound)
  facts = dict(
    _convex_pairs=convex_pairs, _epa_iterations=epa_iterations, epa_iterations=epa_iterations, _heavy_pairs=heavy,
    heavy_colliders=heavy,  # c_model() adds the broadphase options (they may be changed after put_model)
    npolygonmax=npolygonmax, nmeshdegmax=nmeshdegmax, nmaxcondim=nmaxcondim, nmaxpyramid=max(1, 2 * (nmaxcondim - 1)),
    cg_basis=int(pair_condims <= {1, 3} and not has_floss), npair=int(len(pairs)), nexplicit=nexplicit,
    ncullgeom=int(len(cull[0])), ncullgroup=int(len(cull[1])), ncullpair=int(len(cull[2])))
  return facts, dict(nxn_geom_pair=pairs, nxn_pairid=pairid, nxn_pairindex=_pair_index(ngeom, pairs),
                     cull_geom=cull[0], cull_group=cull[1], cull_pair=cull[2], cull_list=cull[3])


def _ray_facts(host):
  """Mesh geoms a ray could hit (visible colour: the reference's _ray_eliminate keeps them, ray.py:52) whose mesh carries no triangles
  (Model.mesh_face; a visual mesh whose asset was never loaded has none): rays() and the rangefinder sensor refuse such a model instead
  of silently reporting "no hit".  Meshes with triangles and height fields are intersected (csrc/ray.hpp)."""
  gt, g_rgba, g_mat, g_data, m_rgba = host["geom_type"], host["geom_rgba"], host["geom_matid"], host["geom_dataid"], host["mat_rgba"]
  mesh_nface = _mesh_face_counts(host)
  no_tri = [g for g in range(len(gt)) if int(gt[g]) == int(types.GeomType.MESH) and (m_rgba[g_mat[g], 3] if g_mat[g] >= 0 else g_rgba[g, 3]) != 0.0
            and (g_data[g] < 0 or g_data[g] >= len(mesh_nface) or mesh_nface[g_data[g]] == 0)]
  if no_tri and (host["sensor_type"] == 7).any():
    raise NotImplementedError("rangefinder sensor in a model with visible mesh geoms that have no triangles (Model.mesh_face): rays against those geoms "
                              "would be reported as no hit; make them invisible to rays (rgba alpha 0), load their mesh or drop the sensor")
  # their geom groups (clamped to 0..5 as the ray elimination does): a rays() call whose geomgroup hides all of them is served
  return dict(_ray_unsupported_geoms=len(no_tri), _ray_unsupported_groups=sorted(set(min(5, max(0, int(host["geom_group"][g]))) for g in no_tri)))


def _options(mjm, m):
  """(Option with its integers, Statistic, their host arrays under the ABI names opt_* / stat_*) (reference io.py:392-470)."""
  opt, f32 = mjm.opt, np.float32
  o, s = types.Option(), types.Statistic()
  o._root = s._root = m
  for name in ("integrator", "cone", "solver", "iterations", "ls_iterations", "disableflags", "enableflags"):
    setattr(o, name, int(getattr(opt, name)))
  o.ccd_iterations = int(getattr(opt, "ccd_iterations", 35))
  # reference io.py:631-636: NXN below 250k filtered pairs, SAP above (tile sort below 1000 geoms)
  o.broadphase = (types.BroadphaseType.NXN if m.npair < 250_000 else
                  types.BroadphaseType.SAP_TILE if m.ngeom < 1000 else types.BroadphaseType.SAP_SEGMENTED)
  # the reference's default adds the OBB filter (io.py:405); contacts do not depend on the filter set (every filter is
  # conservative), only Data.ncollision does, and plane + sphere keeps the light collision kernel
  o.broadphase_filter = types.BroadphaseFilter.PLANE | types.BroadphaseFilter.SPHERE
  if m._heavy_pairs:
    # models that run the heavy collision instantiation anyway get the reference's full default (io.py:405): on the ALOHA scene the
    # sphere test alone lets 760 of 9,154 pairs through to GJK (long extrusions, a table-sized box), the box filters 15
    o.broadphase_filter |= types.BroadphaseFilter.AABB | types.BroadphaseFilter.OBB
  o.graph_conditional = False
  o.run_collision_detection = True
  o.warn_overflow = False
  o.contact_sensor_maxmatch = _check_maxmatch(_numeric(mjm, "contact_sensor_maxmatch", CONTACT_SENSOR_MAXMATCH_CAP))
  return o, s, dict(
    opt_timestep=np.array([opt.timestep], dtype=f32),
    # float32 device arithmetic cannot resolve MuJoCo's default 1e-8 (io.py:398-401)
    opt_tolerance=np.array([max(float(opt.tolerance), 1e-6)], dtype=f32),
    opt_ls_tolerance=np.array([opt.ls_tolerance], dtype=f32), opt_gravity=_arr(opt.gravity, f32).reshape(1, 3),
    opt_impratio_invsqrt=np.array([1.0 / np.sqrt(max(float(opt.impratio), types.MJ_MINVAL))], dtype=f32),
    opt_ccd_tolerance=np.array([float(getattr(opt, "ccd_tolerance", 1e-6))], dtype=f32),
    opt_magnetic=_arr(getattr(opt, "magnetic", [0.0, -0.5, 0.0]), f32).reshape(1, 3),
    stat_meaninertia=np.array([mjm.stat.meaninertia], dtype=f32))


def _level_order(parent):
  """(ids in order of depth, stable; where every depth level starts in that order) of a forest given by parent ids: a root's is negative or its own."""
  depth = np.zeros(len(parent), dtype=np.int32)
  for i, p in enumerate(parent):
    depth[i] = 0 if p < 0 or p == i else depth[p] + 1
  return np.argsort(depth, kind="stable").astype(np.int32), np.concatenate([[0], np.cumsum(np.bincount(depth))]).astype(np.int32)


def _tree_tables(mjm):
  """(sizes and flags, host arrays) derived from the kinematic tree: body / dof level orders, subtree counts, last dofs, the kinematic trees and
  the size classes of the per-tree and island solver kernels."""
  nv, nbody = int(mjm.nv), int(mjm.nbody)
  parent = _arr(mjm.body_parentid, np.int32)
  order, leveladr = _level_order(parent)
  subtreenum = np.ones(nbody, dtype=np.int32)
  for b in range(nbody - 1, 0, -1):
    subtreenum[parent[b]] += subtreenum[b]
  for b in range(1, nbody):  # depth-first numbering => each subtree is a contiguous id range
    if parent[b] >= b or not (parent[b] < b < parent[b] + subtreenum[parent[b]]):
      raise ValueError("bodies must be numbered depth-first (MuJoCo order)")
  dofnum, dofadr = _arr(mjm.body_dofnum, np.int32), _arr(mjm.body_dofadr, np.int32)
  lastdof = np.full(nbody, -1, dtype=np.int32)
  for b in range(1, nbody):
    lastdof[b] = dofadr[b] + dofnum[b] - 1 if dofnum[b] > 0 else lastdof[parent[b]]
  dof_parent = _arr(mjm.dof_parentid, np.int32)
  # kinematic trees: dofs of the bodies below one child of the world, contiguous in MuJoCo's depth-first order
  dof_root = np.zeros(nv, dtype=np.int32)
  for i in range(nv):
    dof_root[i] = i if dof_parent[i] < 0 else dof_root[dof_parent[i]]
  roots = sorted(set(int(r) for r in dof_root))
  tree_dofadr = np.array(roots, dtype=np.int32)
  tree_dofnum = np.array([int(np.sum(dof_root == r)) for r in roots], dtype=np.int32)
  dof_treeid = np.array([roots.index(int(r)) for r in dof_root], dtype=np.int32)
  for t, r in enumerate(roots):
    if not (dof_treeid[r : r + tree_dofnum[t]] == t).all():
      raise ValueError("dofs of a kinematic tree must be contiguous (MuJoCo order)")
  body_treeid = np.array([dof_treeid[lastdof[b]] if lastdof[b] >= 0 else -1 for b in range(nbody)], dtype=np.int32)
  ntree, tree_nvmax = len(roots), int(tree_dofnum.max()) if len(roots) else 0
  # size classes of the island kernels: islands of <= 32 dofs run with 32 lanes and ceil(dofs / 4) quarter-rows -- the widest one is a
  # single tree unless two trees together fit --, islands of 33..64 dofs with 64 lanes
  small = sorted(int(n) for n in tree_dofnum if n <= 32)
  widest = max(small) if small else 0
  if len(small) >= 2 and small[0] + small[1] <= 32:
    widest = 32
  nw = max((nv + 31) // 32, 1)
  dofmask = np.zeros((nbody, nw), dtype=np.uint32)
  for b in range(nbody):  # io.py:536-549 body_isdofancestor as bit masks
    dsel = lastdof[b]
    while dsel >= 0:
      dofmask[b, dsel >> 5] |= np.uint32(1 << (dsel & 31))
      dsel = dof_parent[dsel]
  dorder, dleveladr = _level_order(dof_parent)
  jnt_type, jnt_dofadr, dof_jnt = np.asarray(mjm.jnt_type), np.asarray(mjm.jnt_dofadr), np.asarray(mjm.dof_jntid)
  grpadr = np.arange(nv, dtype=np.int32)
  for i in range(nv):
    j = dof_jnt[i]
    if jnt_type[j] == types.JointType.BALL:
      grpadr[i] = jnt_dofadr[j]
    elif jnt_type[j] == types.JointType.FREE and i - jnt_dofadr[j] >= 3:
      grpadr[i] = jnt_dofadr[j] + 3
  facts = dict(
    ntree=ntree, tree_nvmax=tree_nvmax, nbodylevel=len(leveladr) - 1, ndoflevel=len(dleveladr) - 1, isl_nv4=(widest + 3) // 4, isl_wide=int(nv > 32),
    # nv > 64: worlds whose rows each touch one kinematic tree are solved per (world, tree) by the register-resident kernels
    tree_solve=int(nv > 64 and ntree > 1 and tree_nvmax <= 64 and int(mjm.opt.solver) != types.SolverType.PGS))
  return facts, dict(body_lastdof=lastdof, body_subtreenum=subtreenum, body_tree=order, body_leveladr=leveladr, body_dofmask=dofmask,
                     dof_grpadr=grpadr, dof_tree=dorder, dof_leveladr=dleveladr, tree_dofadr=tree_dofadr, tree_dofnum=tree_dofnum,
                     dof_treeid=dof_treeid, body_treeid=body_treeid)


def _check_trn_feedback(trn_feedback, integrator):
  """The kernels that differentiate the actuator force (csrc/integrate.hpp, implicit.hpp, solver.hpp) take one dof per actuator: velocity
  feedback on a multi-dof moment row is refused with the implicit integrators -- at put_model and again when the C struct is built,
  because opt.integrator is read live."""
  if trn_feedback and integrator in (int(types.IntegratorType.IMPLICITFAST), int(types.IntegratorType.IMPLICIT)):
    raise NotImplementedError(f"velocity feedback (an affine gain or bias with a velocity coefficient) on a multi-dof transmission with the "
                              f"{types.IntegratorType(integrator).name.lower()} integrator: the implicit integrators differentiate single-dof rows only; "
                              "use Euler or RK4")
  return integrator


def _actuator_facts(mjm):
  """(facts, host arrays) of the actuators: act_dof_max and act_velfeedback of the single-dof kernels, and the transmission tables of
  csrc/transmission.hpp -- the static sparse structure of Data.actuator_moment (rows in actuator order, columns ascending), its dof-major
  transpose and trn_general, which is 0 exactly when every row is the scalar gear[0] of a hinge / slide joint."""
  nv, nu = int(mjm.nv), int(mjm.nu)
  i32 = lambda n=0, *rest: np.zeros((n, *rest), dtype=np.int32)
  if not nu:
    return dict(act_dof_max=0, act_velfeedback=0, trn_general=0, nJmom=0, trn_feedback=0), dict(
      actuator_trntype=i32(), actuator_trnobj=i32(0, 2), actuator_trnjnt=i32(0, 2), moment_rownnz=i32(), moment_rowadr=i32(), moment_colind=i32(),
      moment_side=i32(), moment_rowid=i32(), momentT_adr=i32(nv + 1), momentT_act=i32(), momentT_ind=i32())
  trntype = _arr(mjm.actuator_trntype, np.int32).reshape(nu)
  tid = _arr(mjm.actuator_trnid, np.int32).reshape(nu, 2)
  for u in range(nu):  # (the kernels index the joint / site tables with these)
    site = trntype[u] == types.TrnType.SITE
    count = int(getattr(mjm, "nsite", 0)) if site else int(mjm.njnt)
    if not 0 <= tid[u, 0] < count or (site and not -1 <= tid[u, 1] < count):
      raise ValueError(f"actuator {u}: actuator_trnid {tid[u].tolist()} does not name a {'site' if site else 'joint'} of the model")
  st = transmission.moment_structure(mjm)
  scalar = st.pop("scalar")
  nJmom = st.pop("nJmom")
  trnid = _arr(mjm.actuator_trnid, np.int32).reshape(nu, 2)
  # what the single-dof kernels (integrate.hpp, implicit.hpp, solver.hpp: d qfrc_actuator / d qvel) index jnt_dofadr with: the target joint
  # of a scalar row; for any other row -- which contributes nothing there, see the refusal below -- the joint of its first dof (0 if empty)
  first, has = np.zeros(nu, dtype=np.int64), st["moment_rownnz"] > 0
  first[has] = st["moment_colind"][st["moment_rowadr"][has]]
  trnjnt = trnid.copy()
  trnjnt[~scalar, 0] = _arr(mjm.dof_jntid, np.int32).reshape(-1)[first[~scalar]]
  trnjnt[~scalar, 1] = -1
  adof = np.asarray(mjm.jnt_dofadr)[trnid[scalar, 0]]
  # d(force)/d(velocity) of an actuator = gainprm[2] * ctrl (affine gain) + biasprm[2] (affine bias): non-positive for every ctrl only
  # without a gain term and with biasprm[2] <= 0 (a position servo's -kv); otherwise the implicitfast matrix can lose definiteness
  gp, bp = np.asarray(mjm.actuator_gainprm, dtype=np.float64).reshape(nu, -1), np.asarray(mjm.actuator_biasprm, dtype=np.float64).reshape(nu, -1)
  gt, bt = np.asarray(mjm.actuator_gaintype).reshape(-1), np.asarray(mjm.actuator_biastype).reshape(-1)
  feedback = ((gt == 1) & (gp[:, 2] != 0.0)) | ((bt == 1) & (bp[:, 2] != 0.0))
  _check_trn_feedback(int((feedback & ~scalar).any()), int(mjm.opt.integrator))
  facts = dict(act_dof_max=int(np.bincount(adof, minlength=max(nv, 1)).max()),
               act_velfeedback=int(bool(((gt == 1) & (gp[:, 2] != 0.0)).any() or ((bt == 1) & (bp[:, 2] > 0.0)).any())),
               trn_general=int(not scalar.all()), nJmom=int(nJmom), trn_feedback=int((feedback & ~scalar).any()))
  return facts, dict(actuator_trntype=_arr(mjm.actuator_trntype, np.int32).reshape(nu), actuator_trnobj=trnid, actuator_trnjnt=trnjnt, **st)


# Model arrays a host model may lack, and what stands in for them: a value fills the declared shape (a property the model's objects have by
# default); None is an empty table (the model has no such objects).
_OPTIONAL_FIELDS = {
  "geom_matid": -1, "geom_dataid": -1, "body_mocapid": -1, "mesh_graphadr": -1, "site_type": 2, "site_size": 0.005,
  "geom_rgba": [0.5, 0.5, 0.5, 1.0], "tree_sleep_policy": int(types.SleepPolicy.AUTO_ALLOWED), "dof_length": 1,
  "jnt_actfrclimited": 0, "jnt_actgravcomp": 0, "jnt_actfrcrange": 0, "geom_group": 0,
  **dict.fromkeys(
    """mat_rgba mesh_vertadr mesh_vertnum mesh_vert mesh_face mesh_faceadr mesh_graph mesh_polyadr mesh_polynormal mesh_polyvertadr
    mesh_polyvertnum mesh_polyvert mesh_polymapadr mesh_polymapnum mesh_polymap hfield_size hfield_nrow hfield_ncol hfield_adr hfield_data
    sensor_type sensor_datatype sensor_objtype sensor_objid sensor_reftype sensor_refid sensor_dim sensor_adr sensor_cutoff
    sensor_intprm sensor_contact_adr sensor_collision_adr
    pair_dim pair_friction pair_solref pair_solreffriction pair_solimp pair_margin pair_gap site_bodyid site_pos site_quat
    eq_type eq_obj1id eq_obj2id eq_solref eq_solimp eq_data""".split()),
}
# sizes the Model takes from the length of one of its arrays (the host model's own counters are not consulted)
_SIZE_FROM_ARRAY = {"nsensor": "sensor_type", "nmesh": "mesh_vertadr", "nmeshvert": "mesh_vert", "nmeshface": "mesh_face", "nmeshpoly": "mesh_polyvertnum",
                    "nmeshgraph": "mesh_graph", "nmeshpolyvert": "mesh_polyvert", "nmeshpolymap": "mesh_polymap", "nhfield": "hfield_nrow",
                    "nhfielddata": "hfield_data", "nmat": "mat_rgba"}
# ... and -1 in a reshape; so are the site and explicit-pair counts: their optional tables are empty when absent, whatever the counters say
_FREE_SIZES = dict.fromkeys([*_SIZE_FROM_ARRAY, "nsite", "nexplicit"], -1)


def _host_array(mjm, name, sizes):
  """The host model's array `name` in the dtype and shape types.Model declares ('*' = 1), or its _OPTIONAL_FIELDS stand-in."""
  shape, dtype, _ = _MODEL_ARRAYS[name]
  dims = lambda env: [1 if n == "*" else n for n in types.eval_shape(shape, env)]
  src = getattr(mjm, name, None)
  if src is None:
    if name not in _OPTIONAL_FIELDS:
      raise AttributeError(f"model is missing field {name}")
    fill = _OPTIONAL_FIELDS[name]
    src = np.zeros(0) if fill is None else np.broadcast_to(fill, dims(sizes))
  return _arr(src, dtype).reshape(dims({**sizes, **_FREE_SIZES}))


def _sensor_facts(sensor_type):
  """Counts of the sensor classes the stages of csrc/sensor.hpp are launched for."""
  supported = set(mjcf_SENS.values())
  bad = [int(t) for t in sensor_type if int(t) not in supported]
  if bad:  # (sensors do not enter the dynamics: the model still loads, their sensordata slots stay zero)
    import warnings

    warnings.warn(f"sensor types {sorted(set(bad))} are not computed by this engine (csrc/sensor.hpp computes {sorted(supported)}): their sensordata entries are 0")
  count = lambda kinds: int(sum(int(t) in kinds for t in sensor_type))
  return dict(nsensor_acc=count((0, 1, 4, 5, 22, 33, 34, 42)), nsensor_energy=count((43, 44)), nsensor_frc=count((4, 5)), nsensor_subtree=count((36, 37)),
              nsensor_contact=count((42,)), nsensor_collision=count((39, 40, 41)))


_SENSOR_ACC_TYPES = (0, 1, 4, 5, 22, 33, 34, 42)  # what the acceleration-stage launches write (csrc/sensor.hpp k_sensor stage 1, k_sensor_contact)


def _history_facts(mjm, nu, sensor_type, sensor_dim, names=None):
  """(facts, host arrays) of the actuator / sensor delays (csrc/history.hpp).  Every name is read from the host model with a default -- a model
  without them has no history.  The buffer addresses are this engine's own layout (mjcf.history_layout: actuators, then sensors, in id order,
  MuJoCo's); a host model that brings addresses must agree with it.  Per sensor stage the ids of the sensors with a buffer, in the order the
  stage's launches of csrc/sensor.hpp serve them.  Refused: a sensor interval, a delay without samples."""
  ns = len(sensor_type)

  def get(name, shape, dtype):
    src = getattr(mjm, name, None)
    if src is None or shape[0] == 0:  # (no such table, or no actuators / sensors for it to describe)
      return np.zeros(shape, dtype=dtype)
    if np.asarray(src).size != int(np.prod(shape)):
      raise ValueError(f"{name} has {np.asarray(src).size} entries, expected shape {shape}")
    return np.ascontiguousarray(np.asarray(src).reshape(shape), dtype=dtype)

  ah, sh = get("actuator_history", (nu, 2), np.int32), get("sensor_history", (ns, 2), np.int32)
  ad, sd = get("actuator_delay", (nu,), np.float32), get("sensor_delay", (ns,), np.float32)
  interval = get("sensor_interval", (ns, 2), np.float32)
  for kind, hist, delay in (("actuator", ah, ad), ("sensor", sh, sd)):
    for i in range(len(hist)):
      who = f"{kind} {i}" + (f" {names[i]!r}" if kind == "sensor" and names is not None and len(names) > i and names[i] else "")
      if kind == "sensor" and interval[i].any():
        raise NotImplementedError(f"{who}: sensor_interval {interval[i].tolist()} (period / phase sampling of a sensor) is not implemented")
      if hist[i, 0] < 0 or not 0 <= hist[i, 1] <= 2 or delay[i] < 0.0:
        raise ValueError(f"{who}: history (nsample, interp) = {hist[i].tolist()}, delay = {float(delay[i])}: nsample and delay must not be negative, interp is 0, 1 or 2")
      if delay[i] > 0.0 and hist[i, 0] < 1:
        raise ValueError(f"{who}: delay = {float(delay[i])} needs a history buffer, nsample >= 1")
  aadr, sadr, nhistory = history_layout(ah[:, 0], sh[:, 0], sensor_dim)
  for name, mine, nsample in (("actuator_historyadr", aadr, ah[:, 0]), ("sensor_historyadr", sadr, sh[:, 0])):
    theirs = getattr(mjm, name, None)
    if theirs is not None and (np.asarray(theirs).reshape(-1)[nsample > 0] != mine[nsample > 0]).any():
      raise ValueError(f"{name} {np.asarray(theirs).tolist()} is not the layout of Data.history (actuator buffers, then sensor buffers, in id order): {mine.tolist()}")
  if getattr(mjm, "nhistory", None) is not None and int(mjm.nhistory) != nhistory:
    raise ValueError(f"nhistory = {int(mjm.nhistory)} does not agree with the buffers of the model ({nhistory} floats)")
  acc = np.isin(sensor_type, _SENSOR_ACC_TYPES)
  lists = [np.flatnonzero((sh[:, 0] > 0) & sel).astype(np.int32) for sel in (~acc, acc)]
  pad = lambda ids: np.concatenate([ids, np.full(ns - len(ids), -1, dtype=np.int32)])
  facts = dict(nhistory=nhistory, nu_history=int((ah[:, 0] > 0).sum()), nsensor_history_posvel=len(lists[0]), nsensor_history_acc=len(lists[1]))
  return facts, dict(actuator_history=ah, actuator_historyadr=aadr, actuator_delay=ad, sensor_history=sh, sensor_historyadr=sadr, sensor_delay=sd,
                     sensor_interval=interval, sensor_history_posvel=pad(lists[0]), sensor_history_acc=pad(lists[1]))


CONTACT_SENSOR_MAXMATCH_CAP = 64  # csrc/sensor_contact.hpp: one wavefront per world, lane k owns match k


def _check_maxmatch(value):
  value = int(value)
  if value < 1 or value > CONTACT_SENSOR_MAXMATCH_CAP:
    raise ValueError(f"contact_sensor_maxmatch = {value}: must be in 1..{CONTACT_SENSOR_MAXMATCH_CAP} (the contact-sensor kernel keeps the matches of a world's "
                     f"sensor in the {CONTACT_SENSOR_MAXMATCH_CAP} lanes of one wavefront)")
  return value


def _numeric(mjm, name, default):
  """First value of the custom numeric `name` of the host model (reference io.py:409-413), `default` when the model has none: the numpy
  stand-in lists its numerics' names; a mujoco.MjModel answers by name."""
  names = getattr(mjm, "numeric_names", None)
  if names is not None:
    return float(np.asarray(mjm.numeric_data)[int(np.asarray(mjm.numeric_adr)[list(names).index(name)])]) if name in names else default
  try:
    return float(mjm.numeric(name).data[0])
  except (AttributeError, KeyError, TypeError):
    return default


def _contact_sensor_tables(host, nsensor_contact):
  """sensor_intprm [nsensor, 3] and sensor_contact_adr [nsensor] of the model whose other sensor tables are in `host`; checks what
  csrc/sensor_contact.hpp relies on."""
  from .mjcf import contact_slot_size

  stype, n = host["sensor_type"], len(host["sensor_type"])
  intprm = host["sensor_intprm"]
  if intprm.shape[0] != n:
    if nsensor_contact:
      raise ValueError(f"sensor_intprm has {intprm.shape[0]} rows for {n} sensors, and the model has contact sensors")
    intprm = np.zeros((n, 3), dtype=np.int32)
  ids = np.flatnonzero(stype == 42).astype(np.int32)
  count = {0: 0, 1: len(host["body_parentid"]), 2: len(host["body_parentid"]), 5: len(host["geom_bodyid"]), 6: len(host["site_type"])}  # per mjtObj
  for i in ids:
    for which, types_ok in (("obj", (0, 1, 2, 5, 6)), ("ref", (0, 1, 2, 5))):  # (the kernel indexes the body / geom / site tables with these)
      t, k = int(host[f"sensor_{which}type"][i]), int(host[f"sensor_{which}id"][i])
      if t not in types_ok or (t != 0 and not 0 <= k < count[t]):
        raise ValueError(f"contact sensor {i}: sensor_{which}type {t} / sensor_{which}id {k} is not an object of the model a contact sensor can name")
    spec, reduce, num = (int(x) for x in intprm[i])
    if not (0 < spec < 128 and 0 <= reduce <= 3 and num >= 1 and int(host["sensor_dim"][i]) == num * contact_slot_size(spec)):
      raise ValueError(f"contact sensor {i}: sensor_intprm {intprm[i].tolist()} (dataspec, reduce, num) does not agree with sensor_dim {int(host['sensor_dim'][i])}")
  return dict(sensor_intprm=np.ascontiguousarray(intprm, dtype=np.int32), sensor_contact_adr=np.concatenate([ids, np.full(n - len(ids), -1, dtype=np.int32)]))


def _equality_tables(mjm, sizes):
  """eq_type and eq_objtype [neq].  eq_objtype is optional in a host model: JOINT for a joint equality, BODY for a connect.  The ids of a
  connect are checked here: csrc/constraint.hpp indexes the body / site tables with them."""
  eq_type = _host_array(mjm, "eq_type", sizes)
  if getattr(mjm, "eq_objtype", None) is None:
    objtype = np.where(eq_type == types.EqType.JOINT, int(types.ObjType.JOINT), int(types.ObjType.BODY)).astype(np.int32)
  else:
    objtype = _arr(mjm.eq_objtype, np.int32).reshape(-1)
  if objtype.shape != eq_type.shape:
    raise ValueError(f"eq_objtype has {objtype.size} entries, expected neq = {eq_type.size}")
  obj1 = _host_array(mjm, "eq_obj1id", sizes) if eq_type.size else np.zeros(0, dtype=np.int32)
  obj2 = _host_array(mjm, "eq_obj2id", sizes) if eq_type.size else np.zeros(0, dtype=np.int32)
  for e in np.flatnonzero(eq_type == types.EqType.CONNECT):
    if int(objtype[e]) not in (types.ObjType.BODY, types.ObjType.SITE):
      raise ValueError(f"equality {e}: a connect names bodies or sites, not objects of type {int(objtype[e])}")
    n = int(mjm.nbody) if int(objtype[e]) == types.ObjType.BODY else int(getattr(mjm, "nsite", 0))
    if not (0 <= int(obj1[e]) < n and 0 <= int(obj2[e]) < n):
      raise ValueError(f"equality {e}: connect ids {int(obj1[e])}, {int(obj2[e])} are outside the model's {n} {'bodies' if int(objtype[e]) == types.ObjType.BODY else 'sites'}")
  return dict(eq_type=eq_type, eq_objtype=objtype, eq_kind=np.stack([eq_type, objtype]).astype(np.int32))


def _body_geoms(mjm, nbody):
  """body_geomnum / body_geomadr [nbody] from geom_bodyid (a body's geoms are contiguous, MuJoCo's order; adr -1 for a body without geoms):
  the same tables MuJoCo compiles, without asking the host model for them."""
  bodyid = _arr(mjm.geom_bodyid, np.int32).reshape(-1)
  if len(bodyid) and (np.diff(bodyid) < 0).any():
    raise ValueError("geoms must be ordered by body (MuJoCo order)")
  num = np.bincount(bodyid, minlength=nbody).astype(np.int32)
  first = np.searchsorted(bodyid, np.arange(nbody)).astype(np.int32)
  return dict(body_geomnum=num, body_geomadr=np.where(num > 0, first, -1).astype(np.int32))


def _collision_sensor_tables(host, names=None):
  """sensor_collision_adr [nsensor] of the model whose other tables are in `host`; checks what csrc/sensor_collision.hpp relies on and
  refuses the geom pairs it does not serve."""
  stype, n = host["sensor_type"], len(host["sensor_type"])
  ids = np.flatnonzero((stype >= 39) & (stype <= 41)).astype(np.int32)
  nbody, ngeom = len(host["body_parentid"]), len(host["geom_bodyid"])
  gtype, dataid, vertnum = host["geom_type"], host["geom_dataid"], host["mesh_vertnum"]
  PLANE, HFIELD, MESH = int(types.GeomType.PLANE), int(types.GeomType.HFIELD), int(types.GeomType.MESH)
  for i in ids:
    sides = []
    who = f"geom distance sensor {i}" + (f" {names[i]!r}" if names is not None and len(names) > i and names[i] else "")
    for which in ("obj", "ref"):
      t, k = int(host[f"sensor_{which}type"][i]), int(host[f"sensor_{which}id"][i])
      if t not in (1, 5) or not 0 <= k < (nbody if t == 1 else ngeom):
        raise ValueError(f"{who}: sensor_{which}type {t} / sensor_{which}id {k} is not a body or geom of the model")
      adr, num = (int(host["body_geomadr"][k]), int(host["body_geomnum"][k])) if t == 1 else (k, 1)
      if num > 0 and not (0 <= adr and adr + num <= ngeom):
        raise ValueError(f"{who}: body {k} has geoms {adr}..{adr + num - 1} outside the model's {ngeom}")
      sides.append(range(adr, adr + num))
    if int(host["sensor_dim"][i]) != {39: 1, 40: 3, 41: 6}[int(stype[i])]:
      raise ValueError(f"{who}: sensor_dim {int(host['sensor_dim'][i])} does not agree with sensor type {int(stype[i])}")
    if float(host["sensor_cutoff"][i]) < 0.0:
      raise ValueError(f"{who}: negative cutoff")
    for g in (*sides[0], *sides[1]):
      if gtype[g] == HFIELD:
        raise NotImplementedError(f"{who}: height-field geom {g} (distance to a height field is not implemented)")
      if gtype[g] == MESH and (dataid[g] < 0 or dataid[g] >= len(vertnum) or vertnum[dataid[g]] <= 0):
        raise NotImplementedError(f"{who}: mesh geom {g} has no vertices")
    if any(gtype[a] == PLANE for a in sides[0]) and any(gtype[b] == PLANE for b in sides[1]):
      raise NotImplementedError(f"{who}: a plane-plane pair (distance between two planes is not implemented)")
  return dict(sensor_collision_adr=np.concatenate([ids, np.full(n - len(ids), -1, dtype=np.int32)]))


def put_model(mjm, batch_sizes: Optional[dict] = None) -> types.Model:
  """Creates a model on device (reference io.py:259).

  Args:
    mjm: compiled model (mujoco.MjModel, or the numpy stand-in built by mujoco_warp_amd.mjcf).
    batch_sizes: optional {field name: nworld} making "*" fields per-world (domain randomisation).
  """
  opt, nv = mjm.opt, int(mjm.nv)
  pairs, pairid = geom_pairs_with_ids(mjm)
  _check_supported(mjm, pairs)
  m = types.Model()
  for name in ("nq", "nv", "nu", "na", "nbody", "njnt", "ngeom", "nsite", "nkey", "nmocap", "neq", "ntendon", "nsensor", "nmesh", "nflex", "nhfield",
               "ncam", "nlight", "nsensordata"):
    setattr(m, name, int(getattr(mjm, name, 0)))
  m.nC = m.nM = int(np.sum(mjm.M_rownnz)) if nv else 0
  m.is_sparse = False
  m.nv_pad = _get_padded_sizes(nv, 1)[1]
  host = {"M_dense": _m_dense(mjm, nv)}  # ABI name -> numpy array in the declared dtype
  for facts, arrays in (_tree_tables(mjm), _collision_facts(mjm, pairs, pairid), _actuator_facts(mjm)):
    for name, value in facts.items():
      setattr(m, name, value)
    host.update(arrays)
  o, s, arrays = _options(mjm, m)
  host.update(arrays)
  host.update(_body_geoms(mjm, m.nbody))
  sizes = {k: v for k, v in vars(m).items() if isinstance(v, int) and not k.startswith("_")}
  for name in ("sensor_type", "sensor_dim"):
    host[name] = _host_array(mjm, name, sizes)
  facts, arrays = _history_facts(mjm, m.nu, host["sensor_type"], host["sensor_dim"], getattr(mjm, "sensor_names", None))
  for name, value in facts.items():
    setattr(m, name, value)
  host.update(arrays)
  host.update(_equality_tables(mjm, sizes))
  m.has_connect = int((host["eq_type"] == types.EqType.CONNECT).any())
  for name in _MODEL_PTR_FIELDS:
    if name not in host:
      host[name] = _host_array(mjm, name, sizes)
  for size, name in _SIZE_FROM_ARRAY.items():
    setattr(m, size, int(host[name].shape[0]))
  for name, value in {**_sensor_facts(host["sensor_type"]), **_ray_facts(host)}.items():
    setattr(m, name, value)
  host.update(_contact_sensor_tables(host, m.nsensor_contact))
  host.update(_collision_sensor_tables(host, getattr(mjm, "sensor_names", None)))
  m.sleep_enabled = int(bool(int(opt.enableflags) & int(types.EnableBit.SLEEP)) and not (int(opt.disableflags) & int(types.DisableBit.ISLAND)))
  m.opt_sleep_tolerance = float(getattr(opt, "sleep_tolerance", 1e-4))
  if m.sleep_enabled and (host["tree_sleep_policy"] > int(types.SleepPolicy.AUTO_ALLOWED)).any():
    raise NotImplementedError("sleep policies NEVER / ALLOWED / INIT are not implemented (reference types.py:308).")
  if m.sleep_enabled and m.nhistory > 0:
    raise NotImplementedError("actuator / sensor delays (nhistory > 0) with sleeping enabled are not implemented: the wake-by-input test reads ctrl")

  for name, n in (batch_sizes or {}).items():
    key = {"timestep": "opt_timestep", "tolerance": "opt_tolerance", "gravity": "opt_gravity",
           "meaninertia": "stat_meaninertia"}.get(name, name)
    if key not in _BATCHED_MODEL_FIELDS:
      raise ValueError(f"{name} is not a batched ('*') Model field")
    host[key] = np.repeat(host[key][:1], int(n), axis=0)

  # ---- upload; public attribute names follow the reference Model ----
  for name in _MODEL_PTR_FIELDS:
    da = DeviceArray.from_numpy(host[name])
    if name.startswith("opt_"):
      setattr(o, name[4:], da)
    elif name.startswith("stat_"):
      setattr(s, name[5:], da)
    else:
      setattr(m, name, da)
  m.opt, m.stat = o, s
  # (the joint ids behind MjhModel.actuator_trnid, see _actuator_facts; Model.actuator_trnid keeps the targets: the same array unless trn_general)
  m.actuator_trnjnt = DeviceArray.from_numpy(host["actuator_trnjnt"]) if m.trn_general else m.actuator_trnid
  m.nxn_geom_pair_filtered = m.nxn_geom_pair
  m.sensor_interval = DeviceArray.from_numpy(host["sensor_interval"])
  m.eq_type, m.eq_objtype = DeviceArray.from_numpy(host["eq_type"]), DeviceArray.from_numpy(host["eq_objtype"])  # (the library reads eq_kind)
  # (host copies of the buffer layout: make_data / reset_data write the buffers' initial state, the read / init functions check their arguments)
  m._history_buffers = history_buffers(*(host[k] for k in ("actuator_history", "actuator_historyadr", "sensor_history", "sensor_historyadr", "sensor_dim")))
  m._history_host = {k: host[k] for k in ("actuator_history", "sensor_history", "sensor_dim")}
  m._ccd_flags_at_put = int(opt.disableflags)
  m.eq_active0 = _arr(getattr(mjm, "eq_active0", np.zeros(0)), np.int32)
  for name, width in (("key_qpos", m.nq), ("key_qvel", nv), ("key_ctrl", m.nu), ("key_mpos", 3 * m.nmocap), ("key_mquat", 4 * m.nmocap), ("key_act", m.na)):
    setattr(m, name, _arr(getattr(mjm, name, np.zeros((0, width))), np.float32))
  m.key_time = _arr(getattr(mjm, "key_time", np.zeros(0)), np.float32)
  _build_reset_tables(m, host["body_mocapid"])
  m._dirty = True
  m._c = None
  return m


def _m_dense(mjm, nv):
  """[nv, 4 ceil(nv / 4)] address in the CSR M-structure of the dense entry (i, c) (symmetric), -1 where M has no entry."""
  nvr = 4 * ((nv + 3) // 4)
  t = np.full((max(nv, 1), max(nvr, 4)), -1, dtype=np.int32)
  rowadr, rownnz, colind = np.asarray(mjm.M_rowadr), np.asarray(mjm.M_rownnz), np.asarray(mjm.M_colind)
  for i in range(nv):
    for a in range(int(rownnz[i])):
      j = int(colind[rowadr[i] + a])
      t[i, j] = t[j, i] = rowadr[i] + a
  return t[:nv] if nv else t[:0]


def _mesh_face_counts(host):
  """Triangles per mesh (host arrays mesh_face / mesh_faceadr; empty when the model has none), after checking that every index stays
  inside its mesh's vertex block: the ray kernels read the vertices through them."""
  adr, face, nmesh = host["mesh_faceadr"].astype(np.int64), host["mesh_face"].astype(np.int64), len(host["mesh_vertadr"])
  if len(adr) == 0 and len(face) == 0:
    return np.zeros(nmesh, dtype=np.int64)
  if len(adr) != nmesh or (np.diff(np.concatenate([[0], adr, [len(face)]])) < 0).any():
    raise ValueError("mesh_faceadr must have one non-decreasing entry per mesh, within mesh_face")
  num = np.diff(np.concatenate([adr, [len(face)]]))
  vnum = host["mesh_vertnum"]
  for i in range(nmesh):
    f = face[adr[i] : adr[i] + num[i]]
    if len(f) and (f.min() < 0 or f.max() >= vnum[i]):
      raise ValueError(f"mesh {i}: face index outside its {vnum[i]} vertices")
  return num


def _c_disableflags(m):
  # the convex narrowphase's buffers (Model.nmeshdegmax / npolygonmax, Data.ws_ccd) were sized from these two bits at put_model /
  # make_data; the reference re-derives them at every call (collision_convex.py:1226, 1346-1366), this engine cannot: a change needs a new
  # put_model (kernels that branch on the live flags would run past buffers sized for the old ones)
  ccd_bits = int(types.DisableBit.NATIVECCD) | int(types.DisableBit.MULTICCD)
  if (int(m.opt.disableflags) ^ int(m._ccd_flags_at_put)) & ccd_bits:
    raise ValueError("opt.disableflags: NATIVECCD / MULTICCD changed after put_model -- the convex narrowphase's buffers were sized from them; call put_model again")
  return int(m.opt.disableflags)


def _c_heavy_colliders(m):
  bf_ = int(m.opt.broadphase_filter)
  if bf_ & ~0xF:
    raise ValueError(f"unknown broadphase filter bits {bf_:#x}")
  if int(m.opt.broadphase) not in (0, 1, 2):
    raise ValueError(f"unknown broadphase {int(m.opt.broadphase)}")
  if int(m.opt.broadphase) == 0 and m._convex_pairs and int(m.npair) > 0 and int(m.ncullpair) == 0:
    # (io.cull_tables declines models beyond its 16-bit geom / 24-bit pair packing -- put_model picks SAP for those; NXN
    # forced on one would fail every step with MJH_E_ARG in launch_ccd_pre: say so here)
    raise NotImplementedError(f"opt.broadphase = NXN with convex pairs needs the pair-group tables, which hold at most 65535 geoms and 2^24 pairs "
                              f"(this model: {int(m.ngeom)} geoms, {int(m.npair)} pairs): use SAP")
  # (the light instantiation hard-wires plane + sphere and NXN and has no sleep filter)
  return int(bool(m._heavy_pairs or bf_ != 3 or int(m.opt.broadphase) != 0 or m.sleep_enabled))


# pointers of MjhModel that are not the Model attribute of the same name
_C_MODEL_POINTERS = {"actuator_trnid": "actuator_trnjnt"}
# scalars of MjhModel that are not plain Model attributes of the same name
_C_MODEL_SCALARS = {
  **{name: (lambda m, name=name: int(getattr(m.opt, name)))
     for name in ("integrator", "cone", "solver", "iterations", "ls_iterations", "enableflags", "broadphase", "broadphase_filter", "ccd_iterations")},
  "integrator": lambda m: _check_trn_feedback(m.trn_feedback, int(m.opt.integrator)), "disableflags": _c_disableflags, "opt_sleep_tolerance": lambda m: float(m.opt_sleep_tolerance), "heavy_colliders": _c_heavy_colliders,
  "contact_sensor_maxmatch": lambda m: _check_maxmatch(m.opt.contact_sensor_maxmatch),
}


def c_model(m: types.Model):
  """ctypes MjhModel for `m`, rebuilt only when a field was re-bound."""
  if m._c is not None and not m._dirty:
    return m._c
  c = _abi.CModel()
  for name, kind, ptr in _abi.MODEL_FIELDS:
    if ptr:
      src = getattr(m.opt, name[4:]) if name.startswith("opt_") else getattr(m.stat, name[5:]) if name.startswith("stat_") else getattr(m, _C_MODEL_POINTERS.get(name, name))
      setattr(c, name, src.ptr)
      if name in _BATCHED_MODEL_FIELDS:
        setattr(c, name + "_nb", src.shape[0])
    elif not name.endswith("_nb"):
      setattr(c, name, _C_MODEL_SCALARS[name](m) if name in _C_MODEL_SCALARS else int(getattr(m, name)))
  _reset_tables(m)  # (a field was re-bound: the device copies of the keyframe tables follow when it was one of theirs)
  object.__setattr__(m, "_c", c)
  object.__setattr__(m, "_dirty", False)
  return c


def _collide_ccap(npair: int, concap: int) -> int:
  """csrc/collide.hpp collide_ccap: candidate capacity of one world's narrowphase."""
  cap = max(8 * concap, 512)
  return (min(npair, cap) + 3) // 4 * 4


def _ccd_handcap(nworld: int, ccap: int) -> int:
  """csrc/collide.hpp ccd_handcap: EPA entries k_ccd_gjk can hand to k_ccd_epa per step (32 per world on average, at least 4096 or all)."""
  return max(nworld * min(ccap, 32), min(nworld * ccap, 4096))


def _ccd_words(nworld: int, iterations: int, hfield: int, npolygonmax: int, nmeshdegmax: int, ccap: int, npair: int, handcap: Optional[int] = None) -> int:
  """Per-lane words of Data.ws_ccd [nworld, words, 32] such that it holds csrc/convex.hpp ccd_layout(...).total floats: per world the
  height-field prisms' polytopes, the per-candidate result cache and the candidate list; then the EPA hand-over
  records (CCD_HAND_WORDS = 64 each) and the multi-contact buffers of the EPA groups (sized from the model like the reference's,
  collision_convex.py:1346-1366)."""
  it = min(int(iterations), 64)
  poly = 8 * (5 + it) + 5 * (6 + 5 * it) + 24
  cache0 = (poly + 4 * 24 + 7 * 50 + 1) * 32 if hfield else 0
  cand = cache0 + ccap * 24
  bmask = (cand + ccap + 4 + 3) // 4 * 4  # k_broad_mask's bit mask over the pair list (64-pair granules)
  world_stride = (bmask + 2 * ((npair + 63) // 64) + 3) // 4 * 4
  handcap = _ccd_handcap(nworld, ccap) if handcap is None else int(handcap)
  mcw = 0  # (the multi-contact recovery works in LDS)
  hand = (world_stride * nworld + 8 + 2 * ((npair + 63) // 64) + 3) // 4 * 4  # (behind the counters and the convex-pair mask)
  total = hand + handcap * 64 + min(handcap + 7, 16384) * mcw
  return (total + 32 * nworld - 1) // (32 * nworld)


def contact_cap(nconmax: int) -> int:
  """Per-world contact capacity of the collision -> constraint hand-off buffer (twice the average budget)."""
  return int(min(max(2 * nconmax, 16), 256))


def _needs_pgs_big(m: types.Model) -> bool:
  """PGS with more than 64 dofs or elliptic cones runs the generic kernel (csrc/pgs_big.hpp), which keeps J M^-1 in Data.ws_pgsB."""
  return int(m.opt.solver) == int(types.SolverType.PGS) and (m.nv > 64 or int(m.opt.cone) == int(types.ConeType.ELLIPTIC))


def _data_sizes(m: types.Model, nworld, nconmax, njmax, naconmax, handcap=None):
  """Every size the shapes of types.Data / Contact / Constraint name, for a Data of `m` with these capacities.  Workspaces of a kernel
  family the model does not run have a leading size of 0."""
  sizes = {name: int(getattr(m, name)) for name in ("nq", "nv", "nu", "na", "nbody", "njnt", "ngeom", "nsite", "nmocap", "neq", "nC", "ntree", "nsensordata", "nmaxpyramid", "nJmom", "nhistory")}
  sizes["njmax_pad"], sizes["nv_pad"] = _get_padded_sizes(m.nv, njmax)
  concap, tree = contact_cap(nconmax), bool(m.tree_solve)
  sizes.update(
    nworld=nworld, njmax=njmax, naconmax=naconmax, concap=concap,
    ntreeadr=m.ntree + 1 if tree else 0, ntreerow=njmax if tree else 0, ntreedof=m.nv if tree else 0, ntreeworld=nworld if tree else 0,
    nsleepworld=nworld if m.sleep_enabled else 0, npgsworld=nworld if _needs_pgs_big(m) else 0,
    nimpworld=nworld if int(m.opt.integrator) == int(types.IntegratorType.IMPLICIT) else 0, nccdworld=nworld if m._convex_pairs else 0,
    nccdword=_ccd_words(nworld, max(int(m.opt.ccd_iterations), int(m.epa_iterations)), m.nhfield, m.npolygonmax, m.nmeshdegmax,
                        _collide_ccap(int(m.npair), concap), int(m.npair), handcap))
  return sizes


def _alloc_data(m: types.Model, nworld, nconmax, njmax, naconmax, mjd=None, nvmax=None, nccdmax=None, naccdmax=None):
  if nvmax is None:
    nvmax = m.nv
  if nvmax < 0 or nvmax > m.nv:  # reference io.py:1731
    raise ValueError(f"nvmax ({nvmax}) must be in [0, nv ({m.nv})]")
  if nconmax is None:
    nconmax = _default_nconmax(None, mjd)  # at least what the host data already holds (reference io.py:1284-1311)
  if njmax is None:
    njmax = _default_njmax(None, mjd)
  if nconmax < 0:
    raise ValueError("nconmax must be >= 0")
  if njmax < 0:
    raise ValueError("njmax must be >= 0")
  if nworld < 1:
    raise ValueError("nworld must be >= 1")
  if naconmax is None:
    naconmax = nworld * nconmax
  if naconmax < 0:
    raise ValueError("naconmax must be >= 0")
  # nccdmax / naccdmax (reference io.py:1741-1753: CCD contacts per world / in total): the number of penetrating convex pairs k_ccd_gjk can
  # hand to k_ccd_epa per step (Data.nccdhand).  Pairs beyond it are dropped and flagged in Data.overflow (OVF_CCD = 16); WHICH pairs depends
  # on the order the wavefronts reserve their entries, so size it for the scene.  Default: 32 per world on average (csrc/collide.hpp ccd_handcap).
  if nccdmax is not None:
    if nccdmax < 0:
      raise ValueError("nccdmax must be >= 0")
    if nccdmax > nconmax:
      raise ValueError(f"nccdmax ({nccdmax}) must be <= nconmax ({nconmax})")
  if naccdmax is not None and naccdmax < 0:
    raise ValueError("naccdmax must be >= 0")
  handcap = None
  if m._convex_pairs and (naccdmax is not None or nccdmax is not None):
    handcap = max(int(naccdmax) if naccdmax is not None else int(nccdmax) * nworld, 1)
  sizes = _data_sizes(m, nworld, nconmax, njmax, naconmax, handcap)
  d = types.Data()
  d.contact = types.Contact()
  d.efc = types.Constraint()
  d.contact._root = d
  d.efc._root = d
  for name in _DATA_PTR_FIELDS:
    shape, dtype, _ = _DATA_ARRAYS[name]
    _set_data_field(d, name, DeviceArray.zeros(types.eval_shape(shape, sizes), dtype=dtype))
  d.qfrc_inverse = DeviceArray.zeros((nworld, m.nv), dtype="float32")  # (inverse() passes it to mjh_inverse as an argument: MjhData has no member for it)
  d.ws_inverse = DeviceArray.zeros((2, nworld, m.nv), dtype="float32")  # (its invdiscrete scratch, here so that no call of inverse() allocates)
  for name in ("nworld", "naconmax", "njmax", "njmax_pad", "nv_pad", "nsleepworld", "npgsworld", "nimpworld", "nccdworld", "nccdword", "concap"):
    setattr(d, name, sizes[name])
  d.nconmax = nconmax
  # the structure of actuator_moment depends on the model only: the reference's per-world Data arrays are filled once, here
  for name in ("moment_rownnz", "moment_rowadr", "moment_colind"):
    setattr(d, name, DeviceArray.from_numpy(np.ascontiguousarray(np.tile(getattr(m, name).numpy().reshape(1, -1), (nworld, 1)))))
  d.ws_order.assign(np.arange(nworld, dtype=np.int32))
  d.sleep_pass = 0
  d.nvmax = int(nvmax)
  _reset_sleep(m, d, None)
  if m.neq:
    d.eq_active.assign(np.tile(m.eq_active0, (nworld, 1)))
  _reset_mocap(m, d, None)
  _reset_history(m, d, None, 0.0)
  d.nmaxpyramid = m.nmaxpyramid
  d.world_offset = 0
  d.nccdhand = (handcap if handcap is not None else _ccd_handcap(nworld, _collide_ccap(int(m.npair), d.concap))) if d.nccdworld else 0
  d.njmax_nnz = njmax * m.nv
  d._c = None
  d._dirty = True
  return d


def _set_data_field(d, name, arr):
  if name.startswith("contact_"):
    setattr(d.contact, name[8:], arr)
  elif name.startswith("efc_"):
    setattr(d.efc, name[4:], arr)
  else:
    setattr(d, name, arr)


def _get_data_field(d, name):
  if name.startswith("contact_"):
    return getattr(d.contact, name[8:])
  if name.startswith("efc_"):
    return getattr(d.efc, name[4:])
  return getattr(d, name)


def c_data(d: types.Data):
  if d._c is not None and not d._dirty:
    return d._c
  c = _abi.CData()
  for name, kind, ptr in _abi.DATA_FIELDS:
    if ptr:
      setattr(c, name, _get_data_field(d, name).ptr)
    else:
      setattr(c, name, int(getattr(d, name)))
  object.__setattr__(d, "_c", c)
  object.__setattr__(d, "_dirty", False)
  return c


def _model_of(mjm):
  """put_data/make_data take the host model like the reference; cache its device Model."""
  m = getattr(mjm, "_mjh_model", None)
  if m is None:
    m = put_model(mjm)
    try:
      mjm._mjh_model = m
    except AttributeError:
      pass
  return m


def make_data(mjm, nworld: int = 1, nconmax: Optional[int] = None, nccdmax: Optional[int] = None,
              njmax: Optional[int] = None, njmax_nnz: Optional[int] = None, naconmax: Optional[int] = None,
              naccdmax: Optional[int] = None, nvmax: Optional[int] = None) -> types.Data:
  """Creates a data object on device (reference io.py:1680); state = qpos0."""
  m = mjm if isinstance(mjm, types.Model) else _model_of(mjm)
  d = _alloc_data(m, nworld, nconmax, njmax, naconmax, nvmax=nvmax, nccdmax=nccdmax, naccdmax=naccdmax)
  d.qpos.assign(np.tile(m.qpos0.numpy()[0], (nworld, 1)))
  return d


def put_data(mjm, mjd, nworld: int = 1, nconmax: Optional[int] = None, nccdmax: Optional[int] = None,
             njmax: Optional[int] = None, njmax_nnz: Optional[int] = None, naconmax: Optional[int] = None,
             naccdmax: Optional[int] = None, nvmax: Optional[int] = None) -> types.Data:
  """Moves data from host to a device (reference io.py:1890): the single host state is tiled nworld times."""
  m = mjm if isinstance(mjm, types.Model) else _model_of(mjm)
  d = _alloc_data(m, nworld, nconmax, njmax, naconmax, mjd, nvmax=nvmax, nccdmax=nccdmax, naccdmax=naccdmax)
  if m.neq and getattr(mjd, "eq_active", None) is not None:
    d.eq_active.assign(np.tile(np.asarray(mjd.eq_active, dtype=np.int32).reshape(1, -1), (nworld, 1)))
  for name in ("qpos", "qvel", "act", "ctrl", "qacc_warmstart", "qfrc_applied", "xfrc_applied", "mocap_pos", "mocap_quat"):
    if not hasattr(mjd, name):
      continue
    src = np.asarray(getattr(mjd, name), dtype=np.float32)
    dst = getattr(d, name)
    if dst.size:
      dst.assign(np.broadcast_to(src.reshape((1,) + dst.shape[1:]), dst.shape))
  d.time.fill_(float(mjd.time))
  if m.nhistory:  # the host's buffers verbatim (a MuJoCo state drops in); a host data without them: the initial state at its time
    if getattr(mjd, "history", None) is not None and np.asarray(mjd.history).size == m.nhistory:
      d.history.assign(np.tile(np.asarray(mjd.history, dtype=np.float32).reshape(1, -1), (nworld, 1)))
    else:
      _reset_history(m, d, None, float(mjd.time))
  if m.ntree and getattr(mjd, "tree_asleep", None) is not None:  # reference io.py:2010-2012, 2138-2140: the host sleep state, tiled
    asleep = np.asarray(mjd.tree_asleep, dtype=np.int32).reshape(1, -1)
    d.tree_asleep.assign(np.tile(asleep, (nworld, 1)))
    d.tree_awake.assign(np.tile((asleep < 0).astype(np.int32), (nworld, 1)))
    if getattr(mjd, "body_awake", None) is not None:
      d.body_awake.assign(np.tile(np.asarray(mjd.body_awake, dtype=np.int32).reshape(1, -1), (nworld, 1)))
    elif d.body_awake.size and (asleep >= 0).any():
      # (a host MjData without body_awake, e.g. mjcf.MjData with `tree_asleep[:] = arange(ntree)`: derive the tables the first wake /
      # update_sleep stage would produce, sleep.py:171-215 -- the reference's host object carries MuJoCo's own)
      treeid, mocap = m.body_treeid.numpy(), m.body_mocapid.numpy()[m.body_rootid.numpy()]  # (a body welded under a mocap body is posed by it: the root's mocap id, as csrc/sleep.hpp)
      ba = np.where(treeid >= 0, np.where(asleep[0][np.maximum(treeid, 0)] < 0, int(types.SleepState.AWAKE), int(types.SleepState.ASLEEP)),
                    np.where(mocap >= 0, int(types.SleepState.AWAKE), int(types.SleepState.STATIC))).astype(np.int32)
      d.body_awake.assign(np.tile(ba, (nworld, 1)))
      bind = np.concatenate([np.flatnonzero(ba != int(types.SleepState.ASLEEP)), np.zeros(int((ba == int(types.SleepState.ASLEEP)).sum()), dtype=np.int64)]).astype(np.int32)
      d.body_awake_ind.assign(np.tile(bind, (nworld, 1)))
      d.nbody_awake.fill_(int((ba != int(types.SleepState.ASLEEP)).sum()))
      dof_awake = asleep[0][m.dof_treeid.numpy()] < 0
      dind = np.concatenate([np.flatnonzero(dof_awake), np.zeros(int((~dof_awake).sum()), dtype=np.int64)]).astype(np.int32)
      d.dof_awake_ind.assign(np.tile(dind, (nworld, 1)))
      d.nv_awake.fill_(int(dof_awake.sum()))
      d.ntree_awake.fill_(int((asleep < 0).sum()))
  return d


def get_data_into(result, mjm, d: types.Data, world_id: int = 0):
  """Gets data from a device into an existing host MjData-like object (reference io.py:2184)."""
  w = world_id
  for name in ("qpos", "qvel", "act", "ctrl", "qacc_warmstart", "qfrc_applied", "xfrc_applied", "mocap_pos", "mocap_quat", "qacc", "xpos", "xquat",
               "xmat", "xipos", "ximat", "xanchor", "xaxis", "geom_xpos", "geom_xmat", "subtree_com", "cinert", "cdof", "crb",
               "qLD", "qLDiagInv", "cvel", "cdof_dot", "qfrc_bias", "qfrc_passive", "qfrc_spring", "qfrc_damper",
               "qfrc_actuator", "qfrc_smooth", "qacc_smooth", "qfrc_constraint", "qfrc_inverse", "actuator_force", "actuator_length",
               "actuator_velocity", "cacc", "cfrc_int"):
    arr = getattr(d, name).numpy()[w]
    cur = getattr(result, name, None)
    if isinstance(cur, np.ndarray) and cur.size == arr.size:
      cur[...] = arr.reshape(cur.shape)
    else:
      setattr(result, name, arr.astype(np.float64))
  result.qM = d.M.numpy()[w].astype(np.float64)
  result.time = float(d.time.numpy()[w])
  # contacts of this world, in the engine's deterministic per-world order
  ncon, adr = int(d.ws_ncon.numpy()[w]), int(d.ws_conadr.numpy()[w])
  result.ncon = ncon
  sl = slice(adr, adr + ncon)
  result.contact_dist = d.contact.dist.numpy()[sl].astype(np.float64)
  result.contact_pos = d.contact.pos.numpy()[sl].astype(np.float64)
  result.contact_frame = d.contact.frame.numpy()[sl].reshape(ncon, 9).astype(np.float64)
  result.contact_geom = d.contact.geom.numpy()[sl]
  result.contact_dim = d.contact.dim.numpy()[sl]
  result.contact_efc_address = d.contact.efc_address.numpy()[sl]
  nefc = min(int(d.nefc.numpy()[w]), d.njmax)
  result.nefc, result.ne, result.nf, result.nl = nefc, int(d.ne.numpy()[w]), int(d.nf.numpy()[w]), int(d.nl.numpy()[w])
  nv = d.qvel.shape[1]
  result.efc_J = d.efc.J.numpy()[w, :nefc, :nv].astype(np.float64)
  for name in ("pos", "margin", "D", "vel", "aref", "frictionloss", "force"):
    setattr(result, "efc_" + name, getattr(d.efc, name).numpy()[w, :nefc].astype(np.float64))
  for name in ("type", "id", "state"):
    setattr(result, "efc_" + name, getattr(d.efc, name).numpy()[w, :nefc])
  result.solver_niter = np.array([int(d.solver_niter.numpy()[w])])
  for name in ("tree_asleep", "tree_awake", "body_awake"):  # reference io.py:2409-2412
    setattr(result, name, getattr(d, name).numpy()[w].copy())
  result.sensordata = d.sensordata.numpy()[w].astype(np.float64)  # reference io.py: sensordata / energy
  result.energy = d.energy.numpy()[w].astype(np.float64)
  result.history = d.history.numpy()[w].astype(np.float64)  # reference io.py: history


def _state_fields(m, d, sig):
  """(tensor viewed as [nworld, size]) of the components selected by sig, in bit order (reference support.py:674-960)."""
  if sig < 0 or sig >= (1 << int(types.State.NSTATE)):
    raise ValueError(f"invalid state signature {sig} >= 2^mjNSTATE")
  S = types.State
  fields = [(S.TIME, d.time, 1), (S.QPOS, d.qpos, m.nq), (S.QVEL, d.qvel, m.nv), (S.ACT, d.act, m.na), (S.HISTORY, d.history, m.nhistory), (S.WARMSTART, d.qacc_warmstart, m.nv),
            (S.CTRL, d.ctrl, m.nu), (S.QFRC_APPLIED, d.qfrc_applied, m.nv), (S.XFRC_APPLIED, d.xfrc_applied, 6 * m.nbody), (S.EQ_ACTIVE, d.eq_active, m.neq),
            (S.MOCAP_POS, d.mocap_pos, 3 * m.nmocap), (S.MOCAP_QUAT, d.mocap_quat, 4 * m.nmocap)]
  return [(arr, n) for bit, arr, n in fields if (sig & int(bit)) and n > 0]


def state_size(m: types.Model, sig: int) -> int:
  """Number of floats of the state components selected by sig (reference mj_stateSize)."""
  S = types.State
  sizes = {S.TIME: 1, S.QPOS: m.nq, S.QVEL: m.nv, S.ACT: m.na, S.HISTORY: m.nhistory, S.WARMSTART: m.nv, S.CTRL: m.nu, S.QFRC_APPLIED: m.nv, S.XFRC_APPLIED: 6 * m.nbody,
           S.EQ_ACTIVE: m.neq, S.MOCAP_POS: 3 * m.nmocap, S.MOCAP_QUAT: 4 * m.nmocap}
  return int(sum(n for bit, n in sizes.items() if sig & int(bit)))


def _active_mask(active, nworld, device):
  """`active` as a bool tensor [nworld, 1] on `device`.  A DeviceArray or a tensor stays on the device (no host trip); anything else is read
  as a host array of truth values and uploaded."""
  import torch

  t = active.t if isinstance(active, DeviceArray) else active
  if isinstance(t, torch.Tensor):
    t = (t if t.dtype == torch.bool else t.ne(0)).to(device)
  else:
    t = torch.as_tensor(np.asarray(t, dtype=bool), device=device)
  if tuple(t.shape) != (nworld,):
    raise ValueError(f"active must have shape ({nworld},), got {tuple(t.shape)}")
  return t.reshape(nworld, 1)


def get_state(m: types.Model, d: types.Data, state: DeviceArray, sig: int, active=None):
  """Copies the concatenated state components selected by sig (types.State bits) from Data into state [nworld, state_size(m, sig)]
  (reference support.get_state, support.py:674); `active` is an optional per-world mask (host array, DeviceArray or tensor).  Device-to-device
  copies; a mask on the device is used where it is."""
  import torch

  if tuple(state.shape) != (d.nworld, state_size(m, int(sig))):  # (checked before anything is written)
    raise ValueError(f"state must have shape ({d.nworld}, {state_size(m, int(sig))})")
  mask = None if active is None else _active_mask(active, d.nworld, state.t.device)
  adr = 0
  for arr, n in _state_fields(m, d, int(sig)):
    src = arr.t.reshape(d.nworld, n).to(state.t.dtype)
    dst = state.t[:, adr : adr + n]
    dst.copy_(src if mask is None else torch.where(mask, src, dst))
    adr += n


def set_state(m: types.Model, d: types.Data, state: DeviceArray, sig: int, active=None):
  """Copies the concatenated state components selected by sig from state into Data (reference support.set_state, support.py:829); `active` as
  in get_state."""
  import torch

  if tuple(state.shape) != (d.nworld, state_size(m, int(sig))):
    raise ValueError(f"state must have shape ({d.nworld}, {state_size(m, int(sig))})")
  mask = None if active is None else _active_mask(active, d.nworld, state.t.device)
  adr = 0
  for arr, n in _state_fields(m, d, int(sig)):
    dst = arr.t.reshape(d.nworld, n)
    src = state.t[:, adr : adr + n].to(dst.dtype)
    dst.copy_(src if mask is None else torch.where(mask, src, dst))
    adr += n


# ---- reset_data / reset_data_keyframe ---------------------------------------------------------------------------------------------------
# On a GPU the whole reset is ONE launch of csrc/reset.hpp on the current stream: a mask or a key array that lives on the device is read where it
# is, nothing is copied to the host and nothing synchronises, so the call can sit in an RL loop (and in a captured graph: forward.StepGraph).
# On the CPU device (host-logic tests only) the numpy code below does the same edits.
#
# The kernel reads device copies of the keyframe tables and of eq_active0 (host numpy attributes of Model).  They are made at put_model and
# follow a re-binding (`m.key_qpos = new_table`: the _Dirty flag makes c_model look again).  An IN-PLACE edit of a host table
# (`m.key_qpos[0, 2] = 1.0`) is not seen: re-bind the attribute (`m.key_qpos = m.key_qpos.copy()`).
_RESET_HOST_TABLES = {"key_qpos": np.float32, "key_qvel": np.float32, "key_act": np.float32, "key_ctrl": np.float32, "key_mpos": np.float32,
                      "key_mquat": np.float32, "key_time": np.float32, "eq_active0": np.int32}


def _build_reset_tables(m, body_mocapid=None):
  """Device copies of the host tables a reset reads, kept on the Model together with the host arrays they were made from.  body_mocapid: the
  host array at put_model; later rebuilds keep the mocap body list (the body tables are not re-bound field by field)."""
  src = tuple(getattr(m, name, None) for name in _RESET_HOST_TABLES)
  dev = {name: DeviceArray.from_numpy(np.zeros(0) if a is None else a, dtype=dtype) for (name, dtype), a in zip(_RESET_HOST_TABLES.items(), src)}
  prev = getattr(m, "_reset_dev", None)
  if body_mocapid is None and prev is not None:
    dev["mocap_bodyid"] = prev[1]["mocap_bodyid"]
  else:
    mid = np.asarray(m.body_mocapid.numpy() if body_mocapid is None else body_mocapid).reshape(-1)
    dev["mocap_bodyid"] = DeviceArray.from_numpy(np.flatnonzero(mid >= 0)[np.argsort(mid[mid >= 0], kind="stable")], dtype=np.int32)  # mocap-id order
  object.__setattr__(m, "_reset_dev", (src, dev))
  return dev


def _reset_tables(m):
  """{name: DeviceArray} of the keyframe tables, eq_active0 and the mocap body list; rebuilt when one of the host tables was re-bound."""
  cur = getattr(m, "_reset_dev", None)
  if cur is not None and all(getattr(m, name, None) is a for name, a in zip(_RESET_HOST_TABLES, cur[0])):
    return cur[1]
  return _build_reset_tables(m)


def _nkey_mocap(m):
  """Keyframes that carry mocap poses (a host model without key_mpos / key_mquat: none)."""
  if not m.nmocap or getattr(m, "key_mpos", None) is None or getattr(m, "key_mquat", None) is None:
    return 0
  return min(len(m.key_mpos), len(m.key_mquat), int(m.nkey))


def _per_world(x, nworld, what, allow_bool):
  """x -- a numpy array (or anything numpy reads), a DeviceArray or a torch tensor -- checked to be [nworld] of an integer dtype (or bool,
  when allowed); returns the numpy array or the tensor."""
  import torch

  t = x.t if isinstance(x, DeviceArray) else x
  if isinstance(t, torch.Tensor):
    kind = "b" if t.dtype == torch.bool else "f" if (t.dtype.is_floating_point or t.dtype.is_complex) else "i"
  else:
    t = np.asarray(t)
    kind = {"u": "i"}.get(t.dtype.kind, t.dtype.kind)
  if kind != "i" and not (allow_bool and kind == "b"):
    raise ValueError(f"{what} must be of {'bool or ' if allow_bool else ''}integer dtype, got {t.dtype}")
  if tuple(t.shape) != (nworld,):
    raise ValueError(f"{what} must have shape ({nworld},), got {tuple(t.shape)}")
  return t


def _host(t):
  return t if isinstance(t, np.ndarray) else t.detach().cpu().numpy()


def _device_mask(t, device):
  """The checked mask as a contiguous device tensor of one of the dtypes the kernel reads (1-byte or int32 entries)."""
  import torch

  if isinstance(t, np.ndarray):
    return torch.from_numpy(np.ascontiguousarray(t != 0)).to(device)
  if t.dtype not in (torch.bool, torch.uint8, torch.int8, torch.int32):
    t = t.ne(0)
  return t.to(device).contiguous()


def _device_keys(t, nkey, device):
  """The checked per-world keys as a contiguous int32 device tensor (wider integers are clamped to [-1, nkey] first: out of range stays out of range)."""
  import torch

  if isinstance(t, np.ndarray):
    return torch.from_numpy(np.clip(t, -1, nkey).astype(np.int32)).to(device)
  if t.dtype != torch.int32:
    t = t.clamp(-1, nkey).to(torch.int32)
  return t.to(device).contiguous()


def c_reset(m, d, mask=None, keys=None, key=-1):
  """ctypes MjhReset for a reset of `d`: mask / keys are device tensors as _device_mask / _device_keys return them (or None), `key` the scalar
  keyframe (-1: qpos0).  Returns (struct, what it points to -- to be kept alive while a launch or a graph may read it)."""
  import torch

  tabs = _reset_tables(m)
  if keys is not None or key >= 0:  # (the kernel indexes the tables with keys below nkey: a host model that brought fewer rows must not get that far)
    for name, width in (("key_qpos", m.nq), ("key_qvel", m.nv), ("key_act", m.na), ("key_ctrl", m.nu), ("key_time", 1)):
      if width and tabs[name].size != int(m.nkey) * width:
        raise ValueError(f"Model.{name} has {tabs[name].size} entries, expected nkey x {width} = {int(m.nkey) * width}")
    nkm = _nkey_mocap(m)
    if tabs["key_mpos"].size < nkm * 3 * m.nmocap or tabs["key_mquat"].size < nkm * 4 * m.nmocap:
      raise ValueError(f"Model.key_mpos / key_mquat do not hold {nkm} keyframes of {m.nmocap} mocap poses")
  if m.neq and tabs["eq_active0"].size != int(m.neq):
    raise ValueError(f"Model.eq_active0 has {tabs['eq_active0'].size} entries, expected neq = {int(m.neq)}")
  r = _abi.CReset()
  ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
  if mask is not None:
    if mask.dtype == torch.int32:
      r.mask_i32 = ptr(mask)
    else:
      r.mask_u8 = ptr(mask)
  r.keys = ptr(keys)
  r.key, r.nkey, r.nkey_mocap = int(key), int(m.nkey), _nkey_mocap(m)
  for name in (*_RESET_HOST_TABLES, "mocap_bodyid"):
    setattr(r, name, tabs[name].ptr or None)
  return r, (tabs, mask, keys)


def _reset_device(m, d, mask, keys, key):
  from .forward import _stream

  device = d.time.t.device
  mask = None if mask is None else _device_mask(mask, device)
  keys = None if keys is None else _device_keys(keys, int(m.nkey), device)
  r, keep = c_reset(m, d, mask, keys, key)
  _abi.check(_abi.lib().mjh_reset(ctypes.byref(c_model(m)), ctypes.byref(c_data(d)), ctypes.byref(r), _stream()))
  # (`keep`: tensors made here are freed on return; torch's allocator hands their memory out again in stream order, behind the launch)


def _on_gpu(d):
  return d.time.t.device.type != "cpu"


def reset_data(m: types.Model, d: types.Data, reset=None):
  """Resets data to qpos0 (reference io.py:2435).  `reset`: optional per-world mask [nworld] of bool or integer dtype -- a numpy array, a
  DeviceArray or a torch tensor; nonzero entries are reset.  On a GPU: one launch on the current stream, no synchronisation; only a numpy mask
  is uploaded."""
  mask = None if reset is None else _per_world(reset, d.nworld, "reset", True)
  if _on_gpu(d):
    return _reset_device(m, d, mask, None, -1)
  mask = None if mask is None else _host(mask) != 0
  _reset_state(m, d, np.tile(m.qpos0.numpy()[:1], (d.nworld, 1)) if m.qpos0.shape[0] == 1 else m.qpos0.numpy()[np.arange(d.nworld) % m.qpos0.shape[0]],
               None, None, None, 0.0, mask)


def reset_data_keyframe(m: types.Model, d: types.Data, key, reset=None):
  """Resets data to keyframe `key` (reference io.py:2797).  `key`: an int (out of range: ValueError), or one keyframe per world [nworld] of integer
  dtype (numpy array, DeviceArray or torch tensor) -- a world whose key is outside [0, nkey) is not reset.  `reset` as in reset_data; a world is
  reset when both select it.  The keyframe tables are read from their device copies: after an in-place edit of m.key_* re-bind the attribute."""
  keys = None
  if isinstance(key, (int, np.integer)):
    key = int(key)
    if key < 0 or key >= m.nkey:
      raise ValueError(f"keyframe {key} out of range [0, {m.nkey})")
  else:
    keys, key = _per_world(key, d.nworld, "key", False), -1
  mask = None if reset is None else _per_world(reset, d.nworld, "reset", True)
  if _on_gpu(d):
    return _reset_device(m, d, mask, keys, key)
  mask = None if mask is None else _host(mask) != 0
  W = d.nworld
  if keys is None:
    k, time = np.full(W, key), float(m.key_time[key])
  else:
    keys = _host(keys)
    valid = (keys >= 0) & (keys < m.nkey)
    mask = valid if mask is None else mask & valid  # (a mask even when every key is valid: the per-world form never touches the global counters)
    if not mask.any():
      return
    k = np.where(valid, keys, 0)
    time = np.asarray(m.key_time, dtype=np.float32)[k]
  _reset_state(m, d, m.key_qpos[k], m.key_qvel[k], m.key_act[k] if m.na else None, m.key_ctrl[k] if m.nu else None, time, mask)
  nkm = _nkey_mocap(m)
  if nkm and (k < nkm).any():  # keyframe mocap poses (io.py:2855)
    sel = (k < nkm) if mask is None else mask & (k < nkm)
    for name, src, width in (("mocap_pos", m.key_mpos, 3), ("mocap_quat", m.key_mquat, 4)):
      val = np.asarray(src, dtype=np.float32).reshape(len(src), m.nmocap, width)[np.minimum(k, nkm - 1)]
      cur = getattr(d, name).numpy().copy()
      cur[sel] = val[sel]
      getattr(d, name).assign(cur)


def _reset_mocap(m, d, mask):
  """mocap_pos / mocap_quat = the model pose of the mocap bodies (reference io.py:2552 reset_mocap)."""
  if not m.nmocap:
    return
  mid = m.body_mocapid.numpy()
  order = np.argsort(mid[mid >= 0])
  bodies = np.flatnonzero(mid >= 0)[order]
  for name, src in (("mocap_pos", m.body_pos), ("mocap_quat", m.body_quat)):
    val = src.numpy()[np.arange(d.nworld) % src.shape[0]][:, bodies]
    dst = getattr(d, name)
    if mask is None:
      dst.assign(val)
    else:
      cur = dst.numpy().copy()
      cur[mask] = val[mask]
      dst.assign(cur)


def _reset_sleep(m, d, mask):
  """Every tree fully awake (reference io.py:2637-2670 reset_sleep; make_data io.py:1869-1871)."""
  nt, nb, nv = m.ntree, m.nbody, m.nv
  treeid = m.body_treeid.numpy()
  mocap = m.body_mocapid.numpy()[m.body_rootid.numpy()]  # (the root's mocap id, as csrc/sleep.hpp: bodies welded under a mocap body move with it)
  body_awake = np.where(treeid >= 0, int(types.SleepState.AWAKE), np.where(mocap >= 0, int(types.SleepState.AWAKE), int(types.SleepState.STATIC))).astype(np.int32)
  vals = dict(tree_asleep=np.full((d.nworld, nt), -(1 + types.MJ_MINAWAKE), np.int32), tree_awake=np.ones((d.nworld, nt), np.int32),
              body_awake=np.tile(body_awake, (d.nworld, 1)), body_awake_ind=np.tile(np.arange(nb, dtype=np.int32), (d.nworld, 1)),
              dof_awake_ind=np.tile(np.arange(nv, dtype=np.int32), (d.nworld, 1)), ntree_awake=np.full(d.nworld, nt, np.int32),
              nbody_awake=np.full(d.nworld, nb, np.int32), nv_awake=np.full(d.nworld, nv, np.int32), tree_island=np.full((d.nworld, nt), -1, np.int32),
              nisland=np.zeros(d.nworld, np.int32))
  for name, val in vals.items():
    dst = getattr(d, name)
    if dst.size == 0:
      continue
    if mask is not None:
      cur = dst.numpy().copy()
      cur[mask] = val[mask]
      val = cur
    dst.assign(val)


def _reset_history(m, d, mask, time):
  """Data.history of the worlds in `mask` (None: all) in its initial state at `time` (a scalar, or one per world; mjcf.history_row; the
  timestep is the world's own)."""
  if not m.nhistory:
    return
  h = m.opt.timestep.numpy().reshape(-1).astype(np.float64)
  if np.ndim(time) == 0:
    rows = np.stack([history_row(m._history_buffers, m.nhistory, float(time), hw) for hw in h]).astype(np.float32)
    val = rows[np.arange(d.nworld) % len(h)]
  else:  # (one time per world: the per-world keyframes)
    val = np.stack([history_row(m._history_buffers, m.nhistory, float(time[w]), h[w % len(h)]) for w in range(d.nworld)]).astype(np.float32)
  if mask is not None:
    cur = d.history.numpy().copy()
    cur[mask] = val[mask]
    val = cur
  d.history.assign(val)


def _reset_state(m, d, qpos, qvel, act, ctrl, time, mask):
  def put(dst, val):
    if dst.size == 0:
      return
    if val is None:
      val = np.zeros(dst.shape, dtype=np.float32)
    if mask is None:
      dst.assign(val)
    else:
      cur = dst.numpy().copy()
      cur[mask] = np.asarray(val, dtype=cur.dtype)[mask]
      dst.assign(cur)

  put(d.qpos, qpos)
  put(d.qvel, qvel)
  put(d.act, act)
  put(d.ctrl, ctrl)
  put(d.qacc_warmstart, None)
  put(d.qacc, None)
  put(d.qfrc_applied, None)
  put(d.xfrc_applied, None)
  put(d.time, np.full(d.time.shape, time, dtype=np.float32))
  _reset_mocap(m, d, mask)
  _reset_sleep(m, d, mask)
  _reset_history(m, d, mask, time)
  if m.neq:
    put(d.eq_active, np.tile(m.eq_active0, (d.nworld, 1)))
  if mask is None:
    for name in ("nefc", "ne", "nf", "nl", "solver_niter", "overflow", "nacon", "ncollision", "ws_ncon", "ws_conadr", "ws_ncollision"):
      getattr(d, name).zero_()
  else:  # per-world counters of the reset worlds (the global nacon / ncollision are recomputed by the next collision)
    for name in ("nefc", "ne", "nf", "nl", "solver_niter", "overflow", "ws_ncon", "ws_ncollision"):
      dst = getattr(d, name)
      cur = dst.numpy().copy()
      cur[mask] = 0
      dst.assign(cur)


_ENUMS = {"solver": types.SolverType, "integrator": types.IntegratorType, "cone": types.ConeType}


def override_model(model, overrides):
  """Overrides model parameters, e.g. {"opt.solver": "cg"} or ["opt.iterations=10"] (reference io.py:2933).

  Works on the host model (MjModel-like, before put_model) and on a device Model.
  """
  if isinstance(overrides, (list, tuple)):
    ov = {}
    for item in overrides:
      k, v = item.split("=", 1)
      ov[k.strip()] = v.strip()
    overrides = ov
  for key, val in overrides.items():
    obj = model
    parts = key.split(".")
    for p in parts[:-1]:
      obj = getattr(obj, p)
    attr = parts[-1]
    if not hasattr(obj, attr):
      raise ValueError(f"Unrecognized model field: {key}")
    if attr in _ENUMS and isinstance(val, str) and not val.lstrip("-").isdigit():
      val = int(_ENUMS[attr][val.upper()])
    elif attr in ("disableflags", "enableflags") and isinstance(val, str) and not val.lstrip("-").isdigit():
      enum_cls = types.DisableBit if attr == "disableflags" else types.EnableBit
      bits = 0
      for tok in val.split("|"):
        bits |= int(enum_cls[tok.strip().upper()])
      val = bits
    cur = getattr(obj, attr)
    if isinstance(cur, DeviceArray):
      a = np.asarray(val if not isinstance(val, str) else [float(x) for x in val.replace(",", " ").split()], dtype=np.float32)
      if attr == "tolerance":
        a = np.maximum(a, 1e-6)
      cur.assign(np.broadcast_to(a.reshape(-1) if a.ndim else a, cur.shape) if a.size == 1 else a.reshape(cur.shape))
    elif isinstance(cur, (int, np.integer)):
      setattr(obj, attr, int(val))
    elif isinstance(cur, float):
      setattr(obj, attr, float(val))
    elif isinstance(cur, np.ndarray):
      a = np.asarray(val if not isinstance(val, str) else [float(x) for x in val.replace(",", " ").split()], dtype=cur.dtype)
      cur[...] = a.reshape(cur.shape) if a.size == cur.size else a
    else:
      setattr(obj, attr, val)
    if isinstance(model, types.Model) and attr in ("solver", "integrator", "cone"):
      put = {"solver": (types.SolverType.PGS, types.SolverType.CG, types.SolverType.NEWTON), "integrator": (types.IntegratorType.EULER, types.IntegratorType.RK4, types.IntegratorType.IMPLICITFAST),
             "cone": (types.ConeType.PYRAMIDAL, types.ConeType.ELLIPTIC)}[attr]
      if int(getattr(obj, attr)) not in put:
        raise NotImplementedError(f"unsupported {attr} {val}")
    if hasattr(model, "_mjh_model"):
      try:
        del model._mjh_model
      except AttributeError:
        pass


def load_trajectory(npz_path, mjm, mjd) -> np.ndarray:
  """Control sequence of an NPZ recording resampled onto the model timestep, zero-order hold (reference io.py:3067).

  The file holds `ctrl` [n, nu] and `times` [n] (one timestamp per control; the last control is held for the previous
  interval, or one model timestep if there is only one) or [n + 1] (interval boundaries).  Optional `qpos` [1, nq] /
  `qvel` [1, nv] set the initial state of `mjd`.  Returns ctrl [nstep, nu] with nstep = round(duration / timestep);
  control intervals shorter than a timestep may be skipped.
  """
  z = np.load(npz_path)
  ctrl, times = np.asarray(z["ctrl"]), np.asarray(z["times"])
  if ctrl.ndim != 2 or ctrl.shape[0] == 0:
    raise ValueError(f"ctrl must have shape (nstep, nu) with nstep > 0, got {ctrl.shape}")
  if ctrl.shape[1] != mjm.nu:
    raise ValueError(f"ctrl shape {ctrl.shape} does not match model nu={mjm.nu}")
  n = ctrl.shape[0]
  if times.ndim != 1 or times.shape[0] not in (n, n + 1):
    raise ValueError(f"times shape {times.shape} must contain {n} or {n + 1} timestamps")
  if not np.isfinite(times).all():
    raise ValueError("times must be finite")
  if (np.diff(times) <= 0).any():
    raise ValueError("times must be strictly increasing")
  for name, size in (("qpos", mjm.nq), ("qvel", mjm.nv)):
    if name in z.files and z[name].ndim == 2 and z[name].shape[1] == size:
      getattr(mjd, name)[:] = z[name][0]
  dt = float(mjm.opt.timestep)
  if times.shape[0] == n:  # close the last interval
    hold = times[-1] - times[-2] if n > 1 else dt
    times = np.concatenate([times, [times[-1] + hold]])
  nstep = int(np.round((times[-1] - times[0]) / dt))
  sample = times[0] + (np.arange(nstep) + 1e-7) * dt  # nudged off the boundaries so that equal timestamps hold the new control
  return ctrl[np.searchsorted(times, sample, side="right") - 1]
