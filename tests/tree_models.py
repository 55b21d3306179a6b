"""Deterministic generator of kinematic trees for the smooth-dynamics sweep (tests/test_smooth_sweep.py).

A plain helper module like geom_truth.py: `tree_xml(case)` returns MJCF built from a seeded numpy generator, `CASES` names the cases.  Every
case is the smallest model on one side of one boundary of the smooth kernels' size-dependent control flow (csrc/smooth.hpp, the launchers of
csrc/mjhip.hip): body and dof counts are exact targets, set independently of each other and of the tree's shape.

What the generator controls
  shape     chain (every body the child of the previous one) | star (every body a child of one hub) | comb (a spine with a leaf on every
            vertebra) | forest (separate trees under the world, each a random tree of a given body and dof count) | random (test_fuzz.py's
            pop-back rule)
  joints    0 .. 4 dofs per body from 0 .. 4 joints (6 from a free joint on some tree roots): welded bodies (no joint: body_lastdof and the
            dof-ancestor rows then differ from the body tree), hinge, slide, hinge + slide, ball (with a non-zero pos), slide + slide + hinge,
            ball + hinge, slide + slide + hinge + hinge
  physics   random body pos / quat and joint pos / axis; armature, damping; stiffness with springref on hinge and slide joints, stiffness on
            ball and free joints; gravcomp on every third body and actuatorgravcomp on one joint; capsule geoms from fromto (inertial frames
            off the body frame), a second geom on every fourth body, an explicit <inertial> with a rotated quat on every seventh; a site on every
            third body
  actuators an odd number on hinge / slide joints: motors, position servos with kv and one `general` with filter dynamics (na = 1)
  no rows   <flag contact="disable"/>, no limits, no equalities, no friction loss: nefc = 0 in every world
"""

import numpy as np

# dofs -> joint stacks of that many dofs (joint type names; "ball" = 3 dofs, "free" = 6)
_STACKS = {
  0: [()],
  1: [("hinge",), ("slide",), ("hinge",)],
  2: [("hinge", "slide"), ("hinge", "hinge")],
  3: [("ball",), ("slide", "slide", "hinge")],
  4: [("ball", "hinge"), ("slide", "slide", "hinge", "hinge")],
  6: [("free",)],
}

# name: shape, nbody (world included), nv, seed [, trees (forest: (bodies, dofs) per tree), one_joint (one hinge or slide joint on every body), free (a free joint on the first root; default: when the dofs allow),
#       armature (range; default .02 .. .08), link (scale of the parent-child offsets)]
CASES = {
  # 16 lanes per world in k_mid up to 16 bodies AND 16 dofs (mjhip.hip lanes16), 32 beyond either
  "l16_in": dict(shape="random", nbody=16, nv=16, seed=1),     # k_mid<16> at its limit: every lane of the group has a body and a dof
  "l16_body": dict(shape="random", nbody=17, nv=16, seed=2),   # one body too many: k_mid<32>
  "l16_dof": dict(shape="random", nbody=16, nv=17, seed=3, free=True),   # one dof too many: k_mid<32>
  # 32 lanes up to 32 bodies and dofs; 64 in k_fwd_vel / k_mid beyond either, in k_fwd_pos beyond 32 bodies only (lanes64, launch_pos)
  "l32_in": dict(shape="random", nbody=32, nv=32, seed=4, free=True),   # the last 32-lane model: one full trip
  "l32_body": dict(shape="random", nbody=33, nv=32, seed=5),   # k_fwd_pos<64>, k_fwd_vel<64>, k_mid<64>
  "l32_dof": dict(shape="random", nbody=32, nv=33, seed=6),    # k_fwd_pos<32> with k_fwd_vel<64> (the G1's class); two gravcomp mask words
  "l64_in": dict(shape="random", nbody=64, nv=64, seed=7),     # one full 64-lane trip, two mask words full
  "l64_body": dict(shape="random", nbody=65, nv=64, seed=8, free=True), # a second trip over bodies only
  "l64_dof": dict(shape="random", nbody=64, nv=65, seed=9),    # a second trip over dofs only, a third mask word
  "wide": dict(shape="star", nbody=72, nv=80, seed=10),        # hub + 70 children: one kinematics level wider than the group, subtree sums over 71 ids
  "deep": dict(shape="chain", nbody=41, nv=40, seed=11, one_joint=True, armature=(.2, .4), link=0.5),  # 41 levels (> 32 lanes), dof-ancestor rows up to 40 long (armature: see below)
  "big": dict(shape="random", nbody=101, nv=131, seed=12),     # two trips at 64 lanes (three over dofs), five in the 32-lane factor / solve_m kernels, five mask words
  # (deep: with the default armature (.02 .. .08) and link offsets the float32 build of the oracle misses a quarter of the backward bound of
  # mul_m -- 3.8e-5 against 2.5e-5, cond(M) 4e3 with composite inertias taken about a centre of mass metres away -- so the case has armature
  # .2 .. .4 and half-length links: 3.4e-6, and no row of its M needs a floor above the other cases'.  No launcher refused a case for LDS: none had to shrink.)
  # ld_by_tree (smooth.hpp): nv >= 2 tree_nvmax ceil(ntree max(tree_nvmax - 1, 1) / G)
  "forest_par": dict(shape="forest", nbody=37, nv=48, seed=13, trees=[(3, 4)] * 12),   # 12 trees of 4 dofs: true at G = 32 (48 >= 16) and G = 64 (48 >= 8)
  "forest_seq": dict(shape="forest", nbody=21, nv=30, seed=14, trees=[(12, 18), (8, 12)]),  # two trees: false at G = 32 (30 < 72) and at 64 (30 < 36)
}


def ld_by_tree(ntree, tree_nvmax, nv, G):
  """The switch of csrc/smooth.hpp between the sequential and the tree-parallel L'DL factor / solve, restated."""
  if ntree <= 1:
    return False
  manc = max(tree_nvmax - 1, 1)
  return nv >= 2 * tree_nvmax * ((ntree * manc + G - 1) // G)


def lane_groups(nbody, nv):
  """Lanes per world of (k_fwd_pos, k_fwd_vel, k_mid, k_factor_smooth / k_solve_m) for a model without GJK pairs: the dispatch rules of
  csrc/mjhip.hip (lanes16, lanes64, launch_pos, launch_mid), restated.  The L'DL factor runs in two of them: the `factor_m` stage is
  k_fwd_pos (factor_ld at the first entry's lane count), while `fwd_acceleration` and `forward` publish qLD / qLDiagInv / qacc_smooth from the
  32-lane factor kernel (the last entry), which overwrites what `factor_m` left."""
  l64 = nv > 32 or nbody > 32
  l16 = nv <= 16 and nbody <= 16
  return (64 if l64 and nbody > 32 else 32, 64 if l64 else 32, 16 if l16 else 64 if l64 else 32, 32)


def _parents(r, shape, n, trees):
  """Parent index (-1: the world) of each of n bodies, depth-first numbered."""
  if shape == "chain":
    return [i - 1 for i in range(n)]
  if shape == "star":
    return [-1] + [0] * (n - 1)
  if shape == "comb":  # vertebra, its leaf, next vertebra (child of the vertebra), ...
    return [(-1 if i == 0 else i - 2) if i % 2 == 0 else i - 1 for i in range(n)]

  def popback(n, base):
    out, stack = [], []
    for b in range(n):
      up = int(r.integers(0, len(stack))) if stack else 0  # pop back up the tree, never off its root
      del stack[len(stack) - up:]
      out.append(stack[-1] if stack else -1)
      stack.append(base + b)
    return out

  if shape == "random":
    return popback(n, 0)
  if shape == "forest":
    out = []
    for nb, _ in trees:
      out += popback(nb, len(out))
    assert len(out) == n
    return out
  raise ValueError(shape)


def _dof_counts(r, parent, groups, one_joint, free):
  """(dofs per body: 0 .. 4, or 6 for a free joint on a root, summing to each group's target exactly; {body: stack} of the stacks that must
  occur).  groups: [(body ids, dofs)]."""
  c = np.zeros(len(parent), dtype=int)
  if one_joint:
    c[:] = 1
    return c, {}
  forced = {}
  must = [("slide", "slide", "hinge"), ("ball",)]
  for g, (ids, target) in enumerate(groups):
    ids = list(ids)
    roots = [b for b in ids if parent[b] < 0]
    inner = [b for b in ids if parent[b] >= 0]
    c[ids] = 1
    if len(ids) >= 8:
      for b in inner[2::5]:  # welded bodies, never a root (a welded root would split its tree)
        c[b] = 0
    fixed = set()
    if target - len(ids) >= 4 if free is None else free:
      c[roots[0]] = 6
      fixed.add(roots[0])
    for stack in must[:] if len(groups) == 1 else must[:1]:  # (several groups: one forced stack in each of the first two)
      b = inner[(len(inner) * (1 + len(forced))) // 3]
      c[b] = 3
      fixed.add(b)
      forced[b] = stack
      must.remove(stack)
    guard = 0
    while c[ids].sum() != target:
      b = ids[int(r.integers(0, len(ids)))]
      guard += 1
      assert guard < 100000, "dof target out of reach"
      if b in fixed:
        continue
      lo = 1 if parent[b] < 0 else 0
      if c[ids].sum() < target and c[b] < 4:
        c[b] += 1
      elif c[ids].sum() > target and c[b] > lo:
        c[b] -= 1
  assert not must
  return c, forced


def _f(x):
  return " ".join(f"{v:.4f}" for v in np.atleast_1d(x))


def _unit(r, n=3):
  v = r.standard_normal(n)
  return v / np.linalg.norm(v)


def tree_xml(case):
  """MJCF of a case (a name of CASES or a dict of the same keys)."""
  cfg = CASES[case] if isinstance(case, str) else case
  r = np.random.default_rng(cfg["seed"])
  n = cfg["nbody"] - 1
  one = bool(cfg.get("one_joint"))
  parent = _parents(r, cfg["shape"], n, cfg.get("trees"))
  if cfg["shape"] == "forest":
    groups, at = [], 0
    for nb, nd in cfg["trees"]:
      groups.append((range(at, at + nb), nd))
      at += nb
  else:
    groups = [(range(n), cfg["nv"])]
  ndof, forced = _dof_counts(r, parent, groups, one, cfg.get("free"))
  stacks = [None] * n
  for b in range(n):
    opts = _STACKS[int(ndof[b])]
    stacks[b] = forced.get(b, opts[int(r.integers(0, len(opts)))])
  children = [[] for _ in range(n)]
  for b, p in enumerate(parent):
    if p >= 0:
      children[p].append(b)
  # (what must occur once where the model has the joint for it)
  scalar, state = [], dict(ball_spring=not any("ball" in s for s in stacks), free_spring=not any("free" in s for s in stacks), actgrav=False)
  lines = ['<mujoco>', '<option timestep="0.002"><flag contact="disable"/></option>', "<worldbody>"]

  def emit(b):
    root = parent[b] < 0
    pos = np.array([r.uniform(-1, 1), r.uniform(-1, 1), r.uniform(0.5, 1.5)]) if root else np.append(r.uniform(-.08, .08, 2), -r.uniform(.1, .2)) * cfg.get("link", 1.0)
    gc = ' gravcomp="%.2f"' % r.uniform(0.5, 1.2) if b % 3 == 1 or b == n - 1 else ""  # (the last body: a compensated body below the last dof, hence in the last word of the dof masks)
    lines.append(f'<body name="b{b}" pos="{_f(pos)}" quat="{_f(_unit(r, 4))}"{gc}>')
    if b % 7 == 2:
      lines.append(f'<inertial pos="{_f(r.uniform(-.03, .03, 3))}" quat="{_f(_unit(r, 4))}" mass="{r.uniform(.2, .6):.3f}" diaginertia="{_f(r.uniform(.002, .006, 3))}"/>')
    for k, jt in enumerate(stacks[b]):
      name = f"j{b}_{k}"
      arm = f' armature="{r.uniform(*cfg.get("armature", (.02, .08))):.4f}" damping="{r.uniform(.05, .5):.3f}"'
      if jt == "free":
        spring = ""
        if not state["free_spring"]:
          spring, state["free_spring"] = f' stiffness="{r.uniform(1, 4):.2f}"', True
        lines.append(f'<joint name="{name}" type="free"{arm}{spring}/>')
      elif jt == "ball":
        spring = ""
        if not state["ball_spring"] or r.random() < 0.3:
          spring, state["ball_spring"] = f' stiffness="{r.uniform(.5, 3):.2f}"', True
        lines.append(f'<joint name="{name}" type="ball" pos="{_f(r.uniform(-.05, .05, 3))}"{arm}{spring}/>')
      else:
        extra = ""
        if r.random() < 0.5:
          extra += f' stiffness="{r.uniform(.5, 3):.2f}" springref="{r.uniform(-.2, .2) if jt == "slide" else r.uniform(-20, 20):.3f}"'
        if gc and not state["actgrav"]:
          extra, state["actgrav"] = extra + ' actuatorgravcomp="true"', True
        lines.append(f'<joint name="{name}" type="{jt}" pos="{_f(r.uniform(-.04, .04, 3))}" axis="{_f(_unit(r))}"{arm}{extra}/>')
        scalar.append(name)
    lines.append(f'<geom type="capsule" fromto="0 0 0 {_f(np.append(r.uniform(-.08, .08, 2), -r.uniform(.1, .2)))}" size="{r.uniform(.025, .045):.3f}"/>')
    if b % 4 == 3:
      if r.random() < 0.5:
        lines.append(f'<geom type="sphere" pos="{_f(r.uniform(-.06, .06, 3))}" size="{r.uniform(.03, .05):.3f}"/>')
      else:
        # (spheres and capsules only: a box, ellipsoid or cylinder pair selects the heavy collision instantiation, which pins every kernel to 32 lanes)
        lines.append(f'<geom type="capsule" pos="{_f(r.uniform(-.06, .06, 3))}" quat="{_f(_unit(r, 4))}" size="{_f(r.uniform(.02, .05, 2))}"/>')
    if b % 3 == 0:
      lines.append(f'<site name="s{b}" pos="{_f(r.uniform(-.1, .1, 3))}" quat="{_f(_unit(r, 4))}" size="0.01"/>')
    for c in children[b]:
      emit(c)
    lines.append("</body>")

  for b in range(n):
    if parent[b] < 0:
      emit(b)
  lines.append("</worldbody>")
  assert all(state.values()) and len(scalar) >= 3, (state, len(scalar))
  nu = min(7, len(scalar) if len(scalar) % 2 else len(scalar) - 1)
  at = [int(x) for x in np.linspace(0, len(scalar) - 1, nu).round()]  # spread over the tree: first and last scalar joint included
  lines.append("<actuator>")
  for k, i in enumerate(at):
    if k == 1:
      lines.append(f'<general joint="{scalar[i]}" dyntype="filter" dynprm="{r.uniform(.02, .1):.3f}" gainprm="{r.uniform(1, 3):.2f}" gear="{r.uniform(.5, 2):.2f}"/>')
    elif k % 2:
      lines.append(f'<motor joint="{scalar[i]}" gear="{r.uniform(.5, 3):.2f}"/>')
    else:
      lines.append(f'<position joint="{scalar[i]}" kp="{r.uniform(5, 40):.1f}" kv="{r.uniform(.1, 2):.2f}"/>')
  lines.append("</actuator>")
  lines.append("</mujoco>")
  return "\n".join(lines)
