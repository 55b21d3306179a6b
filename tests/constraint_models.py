"""Deterministic generator of models and states for the constraint-assembly sweep (tests/test_constraint_sweep.py).

A plain helper module like tree_models.py: `constraint_xml(case)` returns MJCF, `CASES` names the cases, `world_state(case, mjm, w)` the
state of world w.  Every case is the smallest model on one side of one boundary of `make_constraint_body<G>` (csrc/constraint.hpp): the four
row sections walk equalities / dofs / joints / contacts in trips of G lanes and rank the active ones with a ballot prefix, the contact rows
are then built in windows of CON_WINDOW = 16 staged records, and every row write is guarded by r < njmax.

What a model is made of
  rake    one body on a free joint (dofs 0 .. 5) that carries N spheres above the floor plane.  The sphere centres lie on the body's x axis
          and the states turn the body about z and then about x only, so a centre's height is the body's, whatever the turn: sphere k with
          `level` L_k has radius 0.05 - UNIT L_k and, in a world `shift`ed by n, dist = UNIT (L_k - n) + UNIT / 2  (UNIT = 4 mm).  Margin and gap
          are multiples of UNIT: the contact is detected when L_k - n <= margin_k + gap_k - 1 (dist < margin + gap) and active when
          L_k - n <= margin_k - 1 (dist < includemargin = margin), and no dist - includemargin comes closer to zero than UNIT / 2 = 2 mm.  The rake string of a case names each sphere's kind in the unshifted
          worlds: A active, I detected but inactive (inside the gap), N not detected.  condim 1 / 3 / 4 / 6 per sphere; spheres have
          priority 1, so a contact takes its sphere's parameters unmixed; `pair`: sphere 0 meets the floor through an explicit <pair> with
          anisotropic friction and solreffriction instead
  arm     a chain of bodies high above the floor whose geoms collide with nothing, `per_body` joints to a body: hinge and slide joints in
          turn, ball joints where the case puts them.  Limited joints have a range and, every second one, a margin; world_state puts each
          below its range, above it, inside it, or inside the margin (active, not yet violated) -- never closer than 1e-3 to a change
  rows    equalities: single-joint ones and two-joint ones with a quartic polycoef in turn, cyclically over the arm's scalar joints (so neq can
          exceed nv), every fourth `active="false"` unless `eq_all`; world_state flips one equality's eq_active in most worlds.  Friction
          loss on every joint (`fl="all"`), none, or on the rake (first dof), the last joint, the first ball joint and every third joint
  params  PSETS in turn on equalities, dofs, joints and spheres: solref positive / negative / with a time constant below 2 timestep (with and,
          `refsafe=False`, without the refsafe clamp); solimp with power 2, 3 and 2.5, a width so small that imp_x > 1, mid at both clamps

World w of a case: shift SHIFTS[w] of the rake; limit pattern "full" (every limited joint active) in the worlds w % 3 == 0 and a mixture in
the others; seeded rake position / turn, velocities, and positions of the joints without a limit.  Worlds 0, 3, 6 .. are the ones whose
counts the case's name states; the others put other counts, ranks and active sets next to them in the same workgroup.
"""

import numpy as np

UNIT = 0.004
NOCONTACT = -10
SHIFTS = (0, 1, -1, 0, 2, NOCONTACT, 0, 1, -1, 0, 1, 0, 0, -1, 2, 0, 0, 1, 0)  # per world; 0 in every world w % 3 == 0

# (solref, solimp)
PSETS = (
  ("0.02 1", "0.9 0.95 0.001 0.5 2"),          # the defaults: power 2, imp_x beyond 1 for most rows
  ("-400 -30", "0.8 0.9 0.05 0.3 3"),          # direct stiffness / damping; power 3, rows on both sides of mid
  ("0.003 0.7", "0.7 0.99 0.0005 0.5 2"),      # time constant below 2 timestep (refsafe); width so small that imp_x > 1
  ("0.05 1.2", "0.5 0.9 0.04 0 3"),            # mid at the lower clamp
  ("0.01 0.9", "0.6 0.95 0.1 1 2.5"),          # mid at the upper clamp, power 2.5
)


def _arm(nscalar, balls=()):
  """Joint types of an arm: nscalar hinge / slide joints in turn, a ball joint in front of the scalar joint of each index in `balls`
  (an index of nscalar: behind the last)."""
  out = []
  for k in range(nscalar + 1):
    out += ["ball"] * list(balls).count(k)
    if k < nscalar:
      out.append("hinge" if k % 2 == 0 else "slide")
  return out


_MIX = "AAIAANAIAA"  # the rake of the general cases: condims 3 1 4 6 3 1 4 6 3 1; in the unshifted worlds the third active contact (record 3) has condim 6
# ("con", a, k): njmax = the first row of the active contact of rank a in world 0, plus k -- (3, 0): exactly between two contacts; (2, 7): inside the
# ten rows of the pyramidal condim-6 contact; window_past = (14, 0) on _CUTRAKE
_CUTS = ("exact", "minus1", "eq", "fric", "limit_ball", ("con", 3, 0), ("con", 2, 7), "window_past")

# name: rake (kinds per sphere), condim (cycled), arm (joint types), neq, eq_all, fl, limited ("all" | "none" | "some"), cone, impratio, refsafe, pair,
#       per_body, cut (how njmax is placed: see test_constraint_sweep.sizes), lanes (k_mid, k_make_constraint: asserted)
CASES = {}


def _case(name, lanes, **kw):
  cfg = dict(rake="", condim=(3, 1, 4, 6), arm=[], neq=0, eq_all=False, fl="some", limited="some", cone="pyramidal", impratio=1, refsafe=True,
             pair=False, per_body=2, cut=None, lanes=lanes, seed=len(CASES) + 1)
  cfg.update(kw)
  CASES[name] = cfg


# ---- 16 lanes in k_mid (nv <= 16 and nbody <= 16), 32 in k_make_constraint -------------------------------------------------------------------
_case("g16_mix", (16, 32), rake=_MIX, arm=_arm(6, (3,)), neq=5)
_case("g16_mix_ell", (16, 32), rake=_MIX, arm=_arm(6, (3,)), neq=5, cone="elliptic", impratio=10, refsafe=False)
_case("g16_neq16", (16, 32), rake="AIA", arm=_arm(10), neq=16, eq_all=True)       # one full trip of k_mid<16> over the equalities, neq = nv
_case("g16_neq17", (16, 32), rake="AIA", arm=_arm(10), neq=17, eq_all=True)       # one lane in a second trip, neq > nv
_case("g16_neq19", (16, 32), rake="AIA", arm=_arm(10), neq=19)                    # inactive ones interleaved: ranks differ from lane numbers
_case("g16_nf16", (16, 32), rake="AIA", arm=_arm(10), fl="all", neq=3)            # a friction row on every dof of a full trip; nf = nv = 16
_case("g16_nf0", (16, 32), rake="AIA", arm=_arm(7, (2,)), fl="none", neq=3)       # no friction rows between equalities and limits
_case("g16_nl16", (16, 32), arm=_arm(16), limited="all", neq=3, fl="all")         # 16 joints, all limited (no rake: ncon = 0 with the other sections full)
_case("g16_nl0", (16, 32), rake="AIA", arm=_arm(7, (2,)), limited="none", neq=3)  # no limit rows between friction and contacts
_case("g16_ncon16", (16, 32), rake="A" * 16, arm=_arm(4), neq=2)                  # one trip of 16 lanes, one full window
_case("g16_ncon17", (16, 32), rake="A" * 17, arm=_arm(4), neq=2, condim=(3, 1, 4, 6, 3, 1, 4, 3, 1, 3, 1, 4, 3, 1, 3, 6, 3))  # contact 15 (condim 6) ends window 0: its rows straddle
_case("g16_act16", (16, 32), rake="A" * 8 + "II" + "A" * 8 + "IN", arm=_arm(4), neq=2)   # 19 detected, 16 active
_case("g16_act17", (16, 32), rake="A" * 8 + "II" + "A" * 9 + "IN", arm=_arm(4), neq=2)   # 20 detected, 17 active
_case("g16_ncon0", (16, 32), rake="NNN", arm=_arm(7, (2,)), neq=3)                # geoms, but no contact in the unshifted worlds
_case("win_ncon32", (16, 32), rake="A" * 32, arm=_arm(4), neq=2, condim=(3, 1, 1, 3))
_case("win_ncon33", (16, 32), rake="A" * 33, arm=_arm(4), neq=2, condim=(3, 1, 1, 3), cone="elliptic")
_case("win_hole", (16, 32), rake="AAA" + "I" * 13 + "I" * 16 + "AAAA", arm=_arm(4), neq=2)   # window 1 holds inactive contacts only
# ---- 32 lanes in both (nv or nbody in 17 .. 32) -----------------------------------------------------------------------------------------------
# (an explicit <pair> selects the collision instantiation that pins every kernel to 32 lanes: the two cases with one are of this class)
_case("g32_mix", (32, 32), rake=_MIX, arm=_arm(14, (5,)), neq=7, pair=True)
_case("g32_mix_ell", (32, 32), rake=_MIX, arm=_arm(14, (5,)), neq=7, pair=True, cone="elliptic", impratio=10, refsafe=False)   # solreffriction on the friction rows
_case("g32_neq32", (32, 32), rake="AIA", arm=_arm(20), neq=32, eq_all=True)
_case("g32_neq33", (32, 32), rake="AIA", arm=_arm(20), neq=33, eq_all=True)
_case("g32_nf32", (32, 32), rake="AIA", arm=_arm(26), fl="all", neq=3)            # nf = nv = 32
_case("g32_nl32", (32, 32), arm=_arm(32), limited="all", neq=3)                   # 32 joints, all limited
_case("g32_ncon32", (32, 32), rake="A" * 32, arm=_arm(14), neq=2, condim=(3, 1, 1, 3))
_case("g32_ncon33", (32, 32), rake="A" * 33, arm=_arm(14), neq=2, condim=(3, 1, 1, 3))
# ---- 64 lanes in both (nv or nbody beyond 32) -------------------------------------------------------------------------------------------------
_case("g64_mix", (64, 64), rake=_MIX, arm=_arm(30, (7, 30)), neq=9)
_case("g64_mix_ell", (64, 64), rake=_MIX, arm=_arm(30, (7, 30)), neq=9, cone="elliptic", impratio=10)
_case("g64_neq64", (64, 64), rake="AIA", arm=_arm(30), neq=64, eq_all=True)
_case("g64_neq65", (64, 64), rake="AIA", arm=_arm(30), neq=65, eq_all=True)
_case("g64_nf64", (64, 64), rake="AIA", arm=_arm(58), fl="all", neq=3)            # nf = nv = 64
_case("g64_nf65", (64, 64), rake="AIA", arm=_arm(59), fl="all", neq=3)            # one lane in a second trip over the dofs
_case("g64_nl64_ball", (64, 64), arm=_arm(63, (63,)), limited="all", neq=3)       # joint 63 is a ball: a ball row as the last row of a trip
_case("g64_nl65", (64, 64), arm=_arm(64, (30,)), limited="all", neq=3)            # 65 joints: one lane in a second trip
_case("g64_ncon64", (64, 64), rake="A" * 64, arm=_arm(30), neq=2, condim=(1, 3, 1, 1))
_case("g64_ncon65", (64, 64), rake="A" * 65, arm=_arm(30), neq=2, condim=(1, 3, 1, 1))
_case("g64_act64", (64, 64), rake=("A" * 7 + "I") * 9 + "A", arm=_arm(30), neq=2, condim=(1, 3, 1, 1))   # 73 detected, 64 active
_case("g64_act65", (64, 64), rake=("A" * 7 + "I") * 9 + "AA", arm=_arm(30), neq=2, condim=(1, 3, 1, 1))  # 74 detected, 65 active
# ---- the njmax cut, at 16 lanes (32 in k_make_constraint) and at 64 ---------------------------------------------------------------------------------
_CUTRAKE = "A" * 14 + "IIAAA"   # active contacts 14 .. 16 are records 16 .. 18: the first active contact of window 1 is rank 14
for _g, _lanes, _a in ((16, (16, 32), _arm(6, (3,))), (64, (64, 64), _arm(30, (7, 30)))):
  for _cut in _CUTS:
    _tag = _cut if isinstance(_cut, str) else f"con{_cut[1]}p{_cut[2]}"
    _case(f"cut{_g}_{_tag}", _lanes, rake=_CUTRAKE if _cut == "window_past" else _MIX, arm=_a, neq=5 if _g == 16 else 9, cut=_cut,
          condim=(1, 3, 1, 1) if _cut == "window_past" else (3, 1, 4, 6))
  _case(f"cut{_g}_ell_con2p2", _lanes, rake=_MIX, arm=_a, neq=5 if _g == 16 else 9, cut=("con", 2, 2), cone="elliptic", impratio=10)  # inside an elliptic condim-6 contact
_case("njmax1024", (16, 32), rake=_MIX, cut=1024)   # the rake alone, 6 dofs: the row tables of con_layout leave room for fewer worlds per workgroup

# ---- what the sections above leave out (appended, so that the seeds of the cases above stay what they were) ------------------------------------------
_case("g32_act32", (32, 32), rake=("A" * 8 + "I") * 4, arm=_arm(14), neq=2, condim=(3, 1, 1, 3))         # 36 detected, 32 active: ranks among inactive ones
_case("g32_act33", (32, 32), rake=("A" * 8 + "I") * 4 + "A", arm=_arm(14), neq=2, condim=(3, 1, 1, 3))   # 37 detected, 33 active
# an empty section between non-empty ones, in every lane class (16 lanes: g16_nf0, g16_nl0, g16_ncon0 above)
_case("g16_neq0", (16, 32), rake="AIA", arm=_arm(7, (2,)))                          # no equality rows in front of friction, limits and contacts
_case("g32_neq0", (32, 32), rake="AIA", arm=_arm(14, (5,)))
_case("g32_nf0", (32, 32), rake="AIA", arm=_arm(14, (5,)), fl="none", neq=3)
_case("g32_nl0", (32, 32), rake="AIA", arm=_arm(14, (5,)), limited="none", neq=3)
_case("g32_ncon0", (32, 32), rake="NNN", arm=_arm(14, (5,)), neq=3)
_case("g64_neq0", (64, 64), rake="AIA", arm=_arm(30, (7, 30)))
_case("g64_nf0", (64, 64), rake="AIA", arm=_arm(30, (7, 30)), fl="none", neq=3)
_case("g64_nl0", (64, 64), rake="AIA", arm=_arm(30, (7, 30)), limited="none", neq=3)
_case("g64_ncon0", (64, 64), rake="NNN", arm=_arm(30, (7, 30)), neq=3)


def _bodies(arm, per_body):
  """The arm's joints (indices into `arm`) body by body: `per_body` scalar joints to a body, a ball joint has a body to itself."""
  out, cur = [], []
  for i, t in enumerate(arm):
    if t == "ball":
      out += ([cur] if cur else []) + [[i]]
      cur = []
    else:
      cur.append(i)
      if len(cur) == per_body:
        out.append(cur)
        cur = []
  return out + ([cur] if cur else [])


def sizes_of(cfg):
  """(nbody, nv, njnt, ngeom) a case's model must have."""
  arm, rake, nb = cfg["arm"], 1 if cfg["rake"] else 0, len(_bodies(cfg["arm"], cfg["per_body"]))
  return (1 + rake + nb, 6 * rake + sum(3 if t == "ball" else 1 for t in arm), rake + len(arm), 1 + len(cfg["rake"]) + nb)


def _f(x):
  return " ".join(f"{v:.6g}" for v in np.atleast_1d(x))


def _sphere(cfg, k):
  """(level, margin, gap) of sphere k in UNITs."""
  kind = cfg["rake"][k]
  margin, gap = ((1, 0), (1, 1), (2, 1))[k % 3] if kind == "A" else (1, 1)
  level = {"A": -(k % 2), "I": margin, "N": margin + gap + 1}[kind]
  return level, margin, gap


def fl_joints(cfg):
  """Indices (in the model's joint order, the rake's free joint first) of the joints with friction loss."""
  arm, rake = cfg["arm"], 1 if cfg["rake"] else 0
  n = rake + len(arm)
  if cfg["fl"] == "all":
    return list(range(n))
  if cfg["fl"] == "none" or n == 0:
    return []
  some = {0, n - 1} | set(range(0, n, 3))
  if "ball" in arm:
    some.add(rake + arm.index("ball"))
  return sorted(some)


def limited_joints(cfg):
  arm, rake = cfg["arm"], 1 if cfg["rake"] else 0
  if cfg["limited"] == "none":
    return []
  return [rake + k for k, t in enumerate(arm) if cfg["limited"] == "all" or t == "ball" or k % 3 != 2]


def constraint_xml(case):
  """MJCF of a case (a name of CASES or a dict of the same keys)."""
  cfg = CASES[case] if isinstance(case, str) else case
  r = np.random.default_rng(cfg["seed"])
  arm, rake = cfg["arm"], cfg["rake"]
  fl, lim = set(fl_joints(cfg)), set(limited_joints(cfg))
  flags = "" if cfg["refsafe"] else '<flag refsafe="disable"/>'
  lines = ["<mujoco>", '<compiler angle="radian"/>',
           f'<option timestep="0.002" cone="{cfg["cone"]}" impratio="{cfg["impratio"]}">{flags}</option>', "<worldbody>",
           '<geom name="floor" type="plane" size="0 0 .05" condim="1" friction="0.01 0.0001 0.00001"/>']
  count = dict(dof=0, jnt=0, geom=0)

  def pset(kind):
    count[kind] += 1
    return PSETS[(count[kind] - 1) % len(PSETS)]

  def joint_attrs(j):
    out = ""
    if j in fl:
      ref, imp = pset("dof")
      out += f' frictionloss="{r.uniform(.05, .4):.3f}" solreffriction="{ref}" solimpfriction="{imp}"'
    return out

  if rake:
    lines.append(f'<body name="rake" pos="0 0 {0.05 + UNIT / 2:.6g}">')
    lines.append(f'<joint name="rake" type="free" armature="0.02"{joint_attrs(0)}/>')
    lines.append('<inertial pos="0 0 0" mass="1.5" diaginertia="0.03 0.04 0.05"/>')
    for k in range(len(rake)):
      level, margin, gap = _sphere(cfg, k)
      ref, imp = pset("geom")
      fr = f"{r.uniform(.3, 1.1):.3f} {r.uniform(.005, .03):.4f} {r.uniform(.0005, .004):.5f}"
      lines.append(f'<geom name="s{k}" type="sphere" pos="{0.03 * (k - (len(rake) - 1) / 2):.6g} 0 0" size="{0.05 - UNIT * level:.6g}" priority="1" '
                   f'condim="{cfg["condim"][k % len(cfg["condim"])]}" friction="{fr}" margin="{UNIT * margin:.6g}" gap="{UNIT * gap:.6g}" solref="{ref}" solimp="{imp}"/>')
    lines.append("</body>")
  j0 = 1 if rake else 0
  scalar = []
  bodies = _bodies(arm, cfg["per_body"])
  for depth, joints in enumerate(bodies):
    pos = "0 1 2" if depth == 0 else _f(np.append(r.uniform(-.05, .05, 2), -r.uniform(.08, .12)))
    lines.append(f'<body name="a{depth}" pos="{pos}">')
    for i in joints:
      j, t = j0 + i, arm[i]
      attrs = f' armature="{r.uniform(.03, .08):.4f}" damping="0.1"' + joint_attrs(j)
      if j in lim:
        ref, imp = pset("jnt")
        rng = "0 0.5" if t == "ball" else ("-0.3 0.4" if t == "hinge" else "-0.05 0.08")
        margin = (0.05 if t == "ball" else 0.02 if t == "hinge" else 0.004) if j % 2 == 0 else 0.0
        attrs += f' limited="true" range="{rng}" margin="{margin}" solreflimit="{ref}" solimplimit="{imp}"'
      if t == "ball":
        lines.append(f'<joint name="j{i}" type="ball" pos="{_f(r.uniform(-.02, .02, 3))}"{attrs}/>')
      else:
        v = r.standard_normal(3)
        lines.append(f'<joint name="j{i}" type="{t}" axis="{_f(v / np.linalg.norm(v))}"{attrs}/>')
        scalar.append(f"j{i}")
    lines.append(f'<geom type="sphere" size="{r.uniform(.03, .05):.3f}" pos="0 0 -0.05" contype="0" conaffinity="0"/>')
  lines += ["</body>"] * len(bodies)
  lines.append("</worldbody>")
  if cfg["pair"] and rake:
    lines.append('<contact><pair geom1="floor" geom2="s0" condim="4" friction="0.9 0.2 0.02 0.003 0.0008" solreffriction="0.05 1.2" '
                 f'margin="{UNIT:.6g}" gap="{UNIT:.6g}" solref="{PSETS[1][0]}" solimp="{PSETS[4][1]}"/></contact>')
  if cfg["neq"]:
    assert scalar, "equalities need scalar joints"
    lines.append("<equality>")
    for e in range(cfg["neq"]):
      ref, imp = PSETS[e % len(PSETS)]
      j1, j2 = scalar[e % len(scalar)], scalar[(3 * e + 1) % len(scalar)]
      active = "" if cfg["eq_all"] or e % 4 != 2 else ' active="false"'
      if e % 2 and j2 != j1:
        lines.append(f'<joint joint1="{j1}" joint2="{j2}" polycoef="{_f(np.append(r.uniform(-.02, .02), r.uniform(-1, 1, 4)))}" solref="{ref}" solimp="{imp}"{active}/>')
      else:
        lines.append(f'<joint joint1="{j1}" polycoef="{r.uniform(-.05, .05):.4f} 0 0 0 0" solref="{ref}" solimp="{imp}"{active}/>')
    lines.append("</equality>")
  lines.append("</mujoco>")
  return "\n".join(lines)


def world_state(case, mjm, w):
  """dict(qpos, qvel, eq_active) of world w: float32-exact float64 arrays (eq_active: int32)."""
  cfg = CASES[case] if isinstance(case, str) else case
  r = np.random.default_rng(7919 * cfg["seed"] + w)
  lim = set(limited_joints(cfg))
  full = w % 3 == 0
  qpos = np.asarray(mjm.qpos0, dtype=np.float64).copy()
  active = 0
  for j in range(mjm.njnt):
    t, a = int(mjm.jnt_type[j]), int(mjm.jnt_qposadr[j])
    margin = float(mjm.jnt_margin[j])
    if t == 0:  # the rake: seeded x, y; the height its shift asks for; turned about z, then about its own x
      qpos[a : a + 2] = r.uniform(-.3, .3, 2)
      qpos[a + 2] = 0.05 + UNIT / 2 - UNIT * SHIFTS[w]
      az, ax = r.uniform(-2, 2), r.uniform(-1, 1)
      qpos[a + 3 : a + 7] = (np.cos(az / 2) * np.cos(ax / 2), np.cos(az / 2) * np.sin(ax / 2), np.sin(az / 2) * np.sin(ax / 2), np.sin(az / 2) * np.cos(ax / 2))
    elif t == 1:
      v = r.standard_normal(3)
      beyond = full or (w + j) % 2 == 0
      angle = (0.7 if beyond else 0.2) if j in lim else r.uniform(.1, 1.)
      qpos[a : a + 4] = np.append(np.cos(angle / 2), np.sin(angle / 2) * v / np.linalg.norm(v))
    elif j in lim:
      lo, hi = (float(x) for x in mjm.jnt_range[j])
      step = 0.03 if t == 3 else 0.006
      modes = ((0, 1, 3) if margin > 0 else (0, 1)) if full else (0, 1, 2, 3)
      mode = modes[(active if full else w + j) % len(modes)]
      active += 1
      u = r.uniform(1, 1.5)  # (no two worlds alike; the nearest any comes to a change of state: a quarter of the slide margin, 1e-3)
      qpos[a] = (lo - u * step, hi + u * step, (lo + hi) / 2 + r.uniform(-step, step), lo + margin * u / 2 if margin > 0 else lo + u * step)[mode]
    else:
      qpos[a] = r.uniform(-.3, .3) if t == 3 else r.uniform(-.04, .04)
  qvel = 0.5 * r.standard_normal(mjm.nv)
  if w == 7:
    qvel[:] = 0.0
  eq = np.asarray(mjm.eq_active0, dtype=np.int32).copy() if mjm.neq else np.zeros(0, dtype=np.int32)
  if mjm.neq and not full:
    eq[(w + w // 3) % mjm.neq] ^= 1
  f32 = lambda x: np.asarray(x, dtype=np.float32).astype(np.float64)
  return dict(qpos=f32(qpos), qvel=f32(qvel), eq_active=eq)
