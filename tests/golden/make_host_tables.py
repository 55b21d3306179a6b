"""Digests of everything put_model / make_data / put_data / c_model / c_data produce on the host side, for a fixed set of models.

tests/golden/host_tables_parent.npz holds them as they were before put_model / make_data were driven from the declared schema
(types.array_fields); tests/test_io_schema.py recomputes them and requires every recorded key to be unchanged.  No GPU is needed:
without one DeviceArray keeps CPU tensors.  Each entry is the first 16 hex digits of the SHA-256 of a field's name, dtype, shape and
bytes (arrays) or of its name, type and repr (scalars); the file stores them as uint64, compressed (9142 entries in 28 KB; 350 KB as text).
Regenerate (only when a host table changes on purpose), from the repo root:
    python tests/golden/make_host_tables.py
"""

import copy
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for _p in (ROOT, os.path.join(ROOT, "tests")):
  if _p not in sys.path:
    sys.path.insert(0, _p)
import conftest  # noqa: E402
import mujoco_warp_amd as mjw  # noqa: E402
from mujoco_warp_amd import _abi, io  # noqa: E402
from mujoco_warp_amd.device import DeviceArray  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "host_tables_parent.npz")
SETTINGS = ((3, 24, 64), (1, 7, 21))  # (nworld, nconmax, njmax)
SCENES = {
  "humanoid": ("humanoid", "humanoid.xml"),
  "three_humanoids": ("humanoid", "three_humanoids.xml"),
  "unitree_g1": ("unitree_g1", "scene_flat.xml"),
  "franka_emika_panda": ("franka_emika_panda", "scene.xml"),
  "aloha_pot": ("aloha_pot", "scene.xml"),
  "clutter_synth": ("clutter_synth", "scene_clutter_synth.xml"),
}
INLINE = {"pendula": conftest.PENDULA_XML, "free_bodies": conftest.FREE_BODIES_XML}


class Hidden:
  """`obj` without the attributes in `names`: what a host model that lacks every optional field looks like to put_model."""

  def __init__(self, obj, names):
    self.__dict__.update(_obj=obj, _names=frozenset(names))

  def __getattr__(self, k):
    if k in self._names:
      raise AttributeError(k)
    return getattr(self._obj, k)


def _digest(name, value):
  h = hashlib.sha256(name.encode())
  if isinstance(value, DeviceArray):
    value = value.numpy()
  if isinstance(value, np.ndarray):
    h.update(f"|{value.dtype}|{value.shape}|".encode())
    h.update(np.ascontiguousarray(value).tobytes())
  else:
    if isinstance(value, (bool, int, np.integer, np.bool_)):
      value = int(value)  # (an IntEnum / IntFlag / bool and the int it equals are the same table entry)
    elif isinstance(value, (float, np.floating)):
      value = float(value)
    h.update(f"|{type(value).__name__}|{value!r}".encode())
  return h.hexdigest()[:16]


def _attrs(obj, prefix, out):
  """Every array and plain value the object carries, public and private (not the cached C struct, the back link or child containers)."""
  for name, value in vars(obj).items():
    if name in ("_c", "_root", "_dirty", "opt", "stat", "contact", "efc"):
      continue
    out[f"{prefix}.{name}"] = _digest(name, value)


def _c_scalars(c, fields, prefix, out):
  for name, kind, ptr in fields:
    if not ptr:
      out[f"{prefix}.{name}"] = _digest(name, getattr(c, name))


def model_tables(m):
  out = {}
  _attrs(m, "Model", out)
  _attrs(m.opt, "Option", out)
  _attrs(m.stat, "Statistic", out)
  _c_scalars(io.c_model(m), _abi.MODEL_FIELDS, "c_model", out)
  return out


def data_tables(d):
  out = {}
  _attrs(d, "Data", out)
  _attrs(d.contact, "Contact", out)
  _attrs(d.efc, "Constraint", out)
  _c_scalars(io.c_data(d), _abi.DATA_FIELDS, "c_data", out)
  return out


def _config(out, name, mjm, batch_sizes=None, key_data=False, settings=SETTINGS):
  m = mjw.put_model(mjm, batch_sizes=batch_sizes)
  out[name] = model_tables(m)
  for nworld, nconmax, njmax in settings:
    if key_data:
      mjd = mjw.mjcf.MjData(mjm)
      if mjm.nkey:
        mjw.mjcf.mj_resetDataKeyframe(mjm, mjd, 0)
      d = mjw.put_data(m, mjd, nworld=nworld, nconmax=nconmax, njmax=njmax)
    else:
      d = mjw.make_data(m, nworld=nworld, nconmax=nconmax, njmax=njmax)
    out[f"{name}@{nworld},{nconmax},{njmax}"] = data_tables(d)


def tables(optional_fields=None):
  """{configuration: {field: digest}} of every configuration of the golden file."""
  optional_fields = io._OPTIONAL_FIELDS if optional_fields is None else optional_fields
  out = {}
  loaded = {name: mjw.mjcf.load_xml(os.path.join(ROOT, "benchmarks", *rel)) for name, rel in SCENES.items()}
  for name, mjm in loaded.items():
    _config(out, name, mjm)
  for name, xml in INLINE.items():
    _config(out, name, mjw.mjcf.from_xml_string(xml), key_data=True)
  for name in ("humanoid", "unitree_g1", "franka_emika_panda"):  # every default of the optional fields
    # (the eq_* tables are optional only in a model without equality constraints: put_model refuses the Panda without them)
    keep = {k for k in optional_fields if k.startswith("eq_")} if loaded[name].neq else set()
    _config(out, name + "/no_optional", Hidden(loaded[name], set(optional_fields) - keep))
  _config(out, "humanoid/batched", loaded["humanoid"], batch_sizes={"gravity": 4, "body_mass": 4})
  pgs = copy.deepcopy(loaded["humanoid"])
  pgs.opt.solver, pgs.opt.cone = int(mjw.SolverType.PGS), int(mjw.ConeType.ELLIPTIC)  # Data.npgsworld
  _config(out, "humanoid/pgs_elliptic", pgs)
  imp = copy.deepcopy(loaded["humanoid"])
  imp.opt.integrator = int(mjw.IntegratorType.IMPLICIT)  # Data.nimpworld
  _config(out, "humanoid/implicit", imp)
  return out


def save(path, tabs):
  """{configuration: {field: digest}} as arrays: the field names once, per configuration the indices of its fields and their digests."""
  keys = sorted({k for fields in tabs.values() for k in fields})
  pos = {k: i for i, k in enumerate(keys)}
  configs = sorted(tabs)
  np.savez_compressed(path, keys=np.array(keys), configs=np.array(configs), start=np.cumsum([0] + [len(tabs[c]) for c in configs]).astype(np.int32),
                      field=np.array([pos[k] for c in configs for k in sorted(tabs[c])], dtype=np.uint16),
                      digest=np.array([int(tabs[c][k], 16) for c in configs for k in sorted(tabs[c])], dtype=np.uint64))


def load(path=OUT):
  z = np.load(path)
  keys, start = z["keys"], z["start"]
  return {str(c): {str(keys[f]): f"{int(d):016x}" for f, d in zip(z["field"][start[i]: start[i + 1]], z["digest"][start[i]: start[i + 1]])}
          for i, c in enumerate(z["configs"])}


if __name__ == "__main__":
  save(OUT, tables())
  print("wrote", OUT)
