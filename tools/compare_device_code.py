#!/usr/bin/env python3
"""Did a change move device code?  Compares the gfx950 code objects of two builds unit by unit, kernel by kernel.

    python tools/compare_device_code.py [--removed <regex>]... <objdir-A> <objdir-B>

<objdir>: a directory holding the builder's objects, `<unit>.o` or the object cache's `<unit>.<key>.o` (build/objcache of a checkout;
build the two commits in separate checkouts so that each has its own).  For every unit of _abi.UNITS: the set of kernel symbols, each
kernel's metadata (the amdhsa.kernels note: VGPR / SGPR / AGPR counts, LDS, scratch, kernarg size, arguments) and its disassembled
instruction stream with addresses stripped (branch targets are relative; the pc-relative offset of another symbol -- the literal of the
s_add_u32 behind an s_getpc_b64 -- moves whenever a unit gains or loses code and is masked).  Exit status 0 when everything is identical -- the bar for a host-only change.
--removed <regex> (repeatable) names kernels that B is meant to have dropped: a symbol of A alone that matches one in full is listed, not counted.
Everything else still fails: a kernel only in B, an unnamed kernel only in A, any metadata or code difference, and a regex that matched nothing.
"""

import glob
import os
import re
import struct
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from mujoco_warp_amd._abi import UNITS  # noqa: E402

LLVM = "/opt/rocm/lib/llvm/bin"


def gfx950_elfs(path):
  """The gfx950 code objects bundled in a host object (clang offload bundle: the unbundling of tests/test_isa.py)."""
  b = open(path, "rb").read()
  for mm in re.finditer(b"__CLANG_OFFLOAD_BUNDLE__", b):
    i = mm.start()
    p = i + 24
    nb = struct.unpack("<Q", b[p:p + 8])[0]
    p += 8
    for _ in range(nb):
      off, size, tl = struct.unpack("<QQQ", b[p:p + 24])
      p += 24
      triple = b[p:p + tl].decode()
      p += tl
      if "gfx950" in triple:
        yield b[i + off:i + off + size]


def kernels_of(path):
  """{kernel symbol: (metadata text, instruction text)} of one object."""
  out = {}
  for elf in gfx950_elfs(path):
    with tempfile.NamedTemporaryFile(suffix=".elf", delete=False) as f:
      f.write(elf)
    try:
      dis = subprocess.run([LLVM + "/llvm-objdump", "-d", "--no-show-raw-insn", f.name], capture_output=True, text=True, check=True).stdout
      notes = subprocess.run([LLVM + "/llvm-readelf", "--notes", f.name], capture_output=True, text=True, check=True).stdout
    finally:
      os.unlink(f.name)
    code = {}
    for blk in re.split(r"\n(?=[0-9a-f]+ <[^>]+>:)", dis):
      mm = re.match(r"[0-9a-f]+ <([^>]+)>:\n", blk)
      if mm:
        lines = [re.sub(r"\s*//.*$", "", ln).rstrip() for ln in blk[mm.end():].splitlines()]
        for i in range(1, len(lines)):  # the pc-relative offset of another symbol (s_getpc_b64 + s_add_u32 <literal>) is an address: it moves with the unit's layout
          if lines[i - 1].lstrip().startswith("s_getpc_b64"):
            lines[i] = re.sub(r"^(\s*s_add_u32 (s\d+), \2, )\S+$", r"\1<pcrel>", lines[i])
        code[mm.group(1)] = "\n".join(lines)
    meta = {}
    kern = notes[notes.index("amdhsa.kernels:"):] if "amdhsa.kernels:" in notes else ""
    kern = re.split(r"\n(?=amdhsa\.\w+:)", kern)[0]
    for ent in re.split(r"\n(?=  - )", kern)[1:]:
      mm = re.search(r"^\s+\.name:\s+(\S+)", ent, flags=re.M)
      if mm:
        meta[mm.group(1).strip("'\"")] = ent
    for name, ent in meta.items():
      out[name] = (ent, code.get(name, ""))
  return out


def find(objdir, unit):
  hits = sorted(glob.glob(os.path.join(objdir, unit + ".o")) + glob.glob(os.path.join(objdir, unit + ".*.o")))
  if len(hits) != 1:
    raise SystemExit(f"{objdir}: {len(hits)} objects for {unit}")
  return hits[0]


def main(a, b, removed=()):
  bad = 0
  total = 0
  hits = {r: 0 for r in removed}
  for unit in UNITS:
    ka, kb = kernels_of(find(a, unit)), kernels_of(find(b, unit))
    only = []
    for k in sorted(set(ka) ^ set(kb)):
      named = [r for r in removed if k in ka and re.fullmatch(r, k)]
      for r in named:
        hits[r] += 1
      if named:
        print(f"     removed as named: {k}")
      else:
        only.append(k)
    diff_meta = [k for k in sorted(set(ka) & set(kb)) if ka[k][0] != kb[k][0]]
    diff_code = [k for k in sorted(set(ka) & set(kb)) if ka[k][1] != kb[k][1]]
    ninstr = sum(len(v[1].splitlines()) for v in ka.values())
    total += len(ka)
    print(f"{unit:28s} kernels {len(ka):3d} / {len(kb):3d}  instructions {ninstr:8d}  symbols only on one side {len(only)}  metadata differs {len(diff_meta)}  code differs {len(diff_code)}")
    for k in only + diff_meta + diff_code:
      print("    ", k)
    bad += len(only) + len(diff_meta) + len(diff_code)
  for r, n in hits.items():
    print(f"--removed {r}: {n} kernels")
    bad += n == 0
  gone = sum(hits.values())
  print(f"{total} kernels compared: " + ((f"{gone} removed as named, the other " if gone else "") + "device code IDENTICAL" if not bad else f"{bad} DIFFERENCES"))
  return 1 if bad else 0


if __name__ == "__main__":
  args, removed = sys.argv[1:], []
  while len(args) >= 2 and args[0] == "--removed":
    removed.append(args[1])
    args = args[2:]
  if len(args) != 2:
    raise SystemExit(__doc__)
  sys.exit(main(args[0], args[1], removed))
