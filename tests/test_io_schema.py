"""CPU tests of the IO boundary's single source of shapes and dtypes: types.array_fields drives put_model, make_data and put_data."""

import os
import re
import sys

import numpy as np
import pytest

import conftest
import mujoco_warp_amd as mjw
from mujoco_warp_amd import _abi, io, types

sys.path.insert(0, conftest.GOLDEN_DIR)
import make_host_tables  # noqa: E402

_HEADER_DTYPE = {"int": "int32", "float": "float32", "unsigned int": "uint32"}


def test_host_tables_match_the_parent():
  """Everything put_model / make_data / put_data / c_model / c_data produce on the host, field by field (name, dtype, shape, bytes), against
  the digests recorded before they were driven from the schema (tests/golden/make_host_tables.py).  Fields added later are allowed; a
  recorded one must neither change nor disappear."""
  golden = make_host_tables.load()
  now = make_host_tables.tables()
  assert len(golden) == 42 and sum(len(v) for v in golden.values()) > 9000  # (the file itself is whole)
  bad = [(config, field, now.get(config, {}).get(field)) for config, fields in golden.items() for field, digest in fields.items()
         if now.get(config, {}).get(field) != digest]
  assert not bad, f"{len(bad)} host table entries differ from the parent, e.g. {bad[:8]}"


@pytest.mark.parametrize("fields,declared", [(_abi.MODEL_FIELDS, io._MODEL_ARRAYS), (_abi.DATA_FIELDS, io._DATA_ARRAYS)], ids=["MjhModel", "MjhData"])
def test_every_abi_pointer_is_declared(fields, declared):
  """Every pointer of the C structs is a declared array with a shape, the dtype of the header's C type, and a leading '*' exactly when the
  header carries its batch count <name>_nb."""
  batched = {n[:-3] for n, kind, ptr in fields if n.endswith("_nb")}
  pointers = [(n, kind) for n, kind, ptr in fields if ptr]
  assert len(pointers) > 100
  for name, kind in pointers:
    assert name in declared, name
    shape, dtype, host = declared[name]
    assert len(shape) >= 1 and not host, name
    assert dtype == _HEADER_DTYPE[kind], (name, dtype, kind)
    assert (shape[0] == "*") == (name in batched), (name, shape)
  assert batched <= {n for n, kind in pointers}


def test_eval_shape():
  sizes = {"nworld": 3, "nq": 7, "nv": 6, "na": 1}
  assert types.eval_shape(("nworld", "nq+3*nv+2*na"), sizes) == (3, 27)
  assert types.eval_shape(("*", "nv", 3), sizes) == ("*", 6, 3)
  with pytest.raises(NameError):
    types.eval_shape(("len(nq)",), {"nq": (1, 2)})  # (no builtins in reach)
  assert types.array_fields(types.Model)["mesh_face"] == (("nmeshface", 3), "int32", False)


def test_missing_required_field_raises_and_optional_does_not(humanoid):
  assert "body_mass" not in io._OPTIONAL_FIELDS and "geom_rgba" in io._OPTIONAL_FIELDS
  with pytest.raises(AttributeError, match="model is missing field body_mass"):
    mjw.put_model(make_host_tables.Hidden(humanoid, {"body_mass"}))
  m = mjw.put_model(make_host_tables.Hidden(humanoid, {"geom_rgba", "site_size", "sensor_type"}))
  assert m.geom_rgba.shape == (humanoid.ngeom, 4) and (m.geom_rgba.numpy() == [0.5, 0.5, 0.5, 1.0]).all()
  assert m.site_size.shape == (humanoid.nsite, 3) and m.nsensor == 0


def test_row_size_table_matches_the_schema():
  """csrc/dev_common.hpp's MJH_ROW_<field> table (the one statement of a batched field's row size on the C side) has exactly the header's
  <field>_nb fields, and every entry is the product of the shape types.py declares behind '*'.  The sizes are pairwise coprime and prime, so no
  mixed-up size name or factor can give the right product."""
  text = open(os.path.join(os.path.dirname(_abi.__file__), "csrc", "dev_common.hpp")).read()
  text = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
  entries = re.findall(r"^#define MJH_ROW_(\w+)\(m\) (.+)$", text, flags=re.M)
  table = dict(entries)
  assert len(entries) == len(table), "a field is listed twice"
  batched = {n[:-3] for n, kind, ptr in _abi.MODEL_FIELDS if n.endswith("_nb")}
  assert len(batched) == 56 and set(table) == batched
  sizes = {"nq": 7, "nv": 5, "nbody": 11, "njnt": 13, "ngeom": 17, "nsite": 19, "nu": 23, "neq": 29}
  declared = {prefix + n: spec[0] for prefix, cls in (("opt_", types.Option), ("stat_", types.Statistic), ("", types.Model))
              for n, spec in types.array_fields(cls).items()}  # (the ABI names, as io.c_model maps them)
  for name, expr in table.items():
    shape = declared[name]
    assert shape[0] == "*", name
    want = int(np.prod(types.eval_shape(shape[1:], sizes), dtype=np.int64))
    expr = re.sub(r"\(m\)\.(\w+)", r"\1", expr)  # over m only: what is left must be integers and size names
    assert re.fullmatch(r"[\w\s*()]+", expr), (name, expr)
    assert int(eval(expr, {"__builtins__": {}}, sizes)) == want, (name, expr, shape)
