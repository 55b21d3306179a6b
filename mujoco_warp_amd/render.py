"""Batched depth / segmentation cameras (reference render_util.py create_render_context / get_depth / get_segmentation, render.py render):
host mirror over mjh_render / mjh_camera_rays (csrc/render.hpp).

A RenderContext holds the active cameras of a host model (MjModel.camera, compiled from <camera>), the unit pixel directions in the camera
frame, and the output buffers for `nworld` worlds.  `render` writes, per pixel, what `rays()` reports for the pixel's ray: planar depth
(hit distance times -ray_cam.z; 0 where nothing is hit), segmentation (geom id, ObjType.GEOM) or (-1, -1), and optionally the world-frame
surface normal.  Static geoms are hit; the geom groups, and optionally the camera's own body, are filtered as `rays()` filters them.
There is no rasteriser, no colour, no texture and no shadow: `render_rgb` and its relatives raise NotImplementedError.  Only fixed
perspective cameras given by `fovy` are built; other cameras load but cannot be active."""

import ctypes
from typing import Optional, Sequence

import numpy as np

from . import _abi
from . import io
from . import types
from .device import DeviceArray
from .forward import _stream

TILE = 8  # csrc/render.hpp RENDER_TILE: one wavefront per TILE x TILE pixels


def compute_ray(fovy: float, width: int, height: int, znear: float) -> np.ndarray:
  """Unit pixel directions [height * width, 3] (float32) in the camera frame, row 0 on top: render_util.compute_ray's fovy branch.  The
  camera looks along -z with +y up; pixel centres sit at (px + .5) / width, (py + .5) / height of the near-plane rectangle."""
  half_height = znear * np.tan(0.5 * np.deg2rad(fovy))
  half_width = half_height * (float(width) / float(height))
  u = (np.arange(width, dtype=np.float64) + 0.5) / float(width)
  v = (np.arange(height, dtype=np.float64) + 0.5) / float(height)
  x = -half_width + 2.0 * half_width * u
  y = half_height - 2.0 * half_height * v
  dirs = np.stack([np.broadcast_to(x[None, :], (height, width)), np.broadcast_to(y[:, None], (height, width)), np.full((height, width), -znear)], axis=-1)
  dirs = dirs / np.linalg.norm(dirs, axis=-1, keepdims=True)
  return dirs.reshape(-1, 3).astype(np.float32)


class RenderContext:
  """Cameras, pixel rays and output buffers of render() (see create_render_context).  Host tables are numpy arrays under their own names
  (`cam_id`, `cam_bodyid`, `cam_pos`, `cam_quat`, `cam_fovy`, `cam_res`, `depth_adr`, `seg_adr`, `ray`); the outputs are DeviceArrays."""

  def __init__(self):
    self._c = None
    self._keep = []

  def c_render(self):
    """ctypes MjhRender of this context (include/mjhip.h)."""
    if self._c is None:
      dev = lambda a, dt: DeviceArray.from_numpy(np.ascontiguousarray(a, dtype=dt))
      t = dict(cam_bodyid=dev(self.cam_bodyid, np.int32), cam_pos=dev(self.cam_pos, np.float32), cam_quat=dev(self.cam_quat, np.float32),
               cam_res=dev(self.cam_res, np.int32), cam_exclude=dev(self.cam_exclude, np.int32), depth_adr=dev(self.depth_adr, np.int32),
               seg_adr=dev(self.seg_adr, np.int32), tile=dev(self.tile, np.int32), ray=dev(self.ray, np.float32))
      self._keep = t
      c = _abi.CRender()
      c.nworld, c.ncam, c.npixel, c.ntile, c.groupmask = self.nworld, self.ncam, self.npixel, len(self.tile), self.groupmask
      for name, arr in t.items():
        setattr(c, name, arr.ptr)
      for name in ("depth", "seg", "normal", "cam_xpos", "cam_xmat"):
        arr = getattr(self, {"depth": "depth_data", "seg": "seg_data", "normal": "normal_data"}.get(name, name))
        setattr(c, name, arr.ptr if arr is not None else None)
      self._c = c
    return self._c


def _active_cameras(cam, cam_active):
  if cam_active is None:
    return list(range(cam.n))
  cam_active = list(cam_active)
  if not cam_active:
    return []
  if isinstance(cam_active[0], (bool, np.bool_)):
    if len(cam_active) != cam.n:
      raise ValueError(f"cam_active must have length {cam.n} (got {len(cam_active)})")
    return [int(i) for i in np.nonzero(cam_active)[0]]
  if isinstance(cam_active[0], str):
    for name in cam_active:
      if name not in cam.names:
        raise ValueError(f"cam_active: no camera named {name!r} (cameras: {cam.names})")
    return [cam.names.index(name) for name in cam_active]
  if isinstance(cam_active[0], (int, np.integer)):
    ids = [int(x) for x in cam_active]
    if any(i < 0 or i >= cam.n for i in ids):
      raise ValueError(f"cam_active: camera index out of range (the model has {cam.n} cameras)")
    return ids
  raise ValueError(f"Invalid cam_active format: {cam_active}")


def _unrendered_meshes(mjm, groups):
  """Visible mesh geoms in an enabled group whose mesh has no triangles (io._ray_facts: the loader reads a mesh asset only for colliding or
  mass-carrying geoms): (count, their groups)."""
  nface = np.diff(np.concatenate([np.asarray(mjm.mesh_faceadr, dtype=np.int64), [len(mjm.mesh_face)]])) if mjm.nmesh else np.zeros(0, dtype=np.int64)
  bad = []
  for g in range(mjm.ngeom):
    if int(mjm.geom_type[g]) != int(types.GeomType.MESH):
      continue
    mat = int(mjm.geom_matid[g])
    alpha = mjm.mat_rgba[mat][3] if mat >= 0 else mjm.geom_rgba[g][3]
    did = int(mjm.geom_dataid[g])
    group = min(5, max(0, int(mjm.geom_group[g])))
    if alpha != 0.0 and (did < 0 or did >= len(nface) or nface[did] == 0) and group in groups:
      bad.append(group)
  return len(bad), sorted(set(bad))


def create_render_context(mjm, nworld: int = 1, cam_res=None, render_depth=True, render_seg=False, render_normal=False,
                          enabled_geom_groups: Sequence[int] = (0, 1, 2), cam_active=None, exclude_camera_body=False, znear: Optional[float] = None, *,
                          render_rgb=False, use_textures=False, use_shadows=False, flex_render_smooth=False, splat_files=None, **unsupported) -> RenderContext:
  """Render context for `nworld` worlds of host model `mjm` (reference render_util.py:272).

  cam_res: one (width, height) for every active camera, a list with one pair per active camera, or None for the MJCF `resolution`.
  render_depth / render_seg / render_normal: which buffers render() fills (`depth_data [nworld, npixel]`, `seg_data [nworld, npixel, 2]`,
  `normal_data [nworld, npixel, 3]`).  enabled_geom_groups: geom groups (0..5) the cameras see.  cam_active: indices, names or one bool
  per camera of `mjm.camera` (None: all).  exclude_camera_body: a camera does not see the geoms of the body it rides on (one bool, or one
  per active camera).  znear: near-plane distance of the pixel rays' construction (default 0.01 extent; a unit direction does not depend on it)."""
  for name, on in (("render_rgb", render_rgb), ("use_textures", use_textures), ("use_shadows", use_shadows), ("flex_render_smooth", flex_render_smooth), ("splat_files", splat_files)):
    if np.any(on):
      raise NotImplementedError(f"create_render_context({name}=...): colour, textures, shadows, flex and splat rendering are not part of this engine (depth, segmentation and normals are)")
  if unsupported:
    raise NotImplementedError(f"create_render_context: unsupported argument(s) {sorted(unsupported)}")
  cam = getattr(mjm, "camera", None)
  if cam is None:
    raise NotImplementedError("create_render_context needs a host model with a camera record (MjModel.camera: mjcf.load_xml / from_xml_string)")
  if int(nworld) <= 0:
    raise ValueError("nworld must be positive")
  ids = _active_cameras(cam, cam_active)
  for i in ids:
    if cam.unbuilt[i]:
      attr, value = cam.unbuilt[i][0]
      raise NotImplementedError(f"camera {cam.names[i]!r} ({i}): {attr}=\"{value}\" is not rendered (only fixed perspective cameras given by fovy are)")
  groups = sorted(set(int(g) for g in enabled_geom_groups))
  if any(g < 0 or g > 5 for g in groups):
    raise ValueError("enabled_geom_groups must lie in 0..5")
  nbad, bad_groups = _unrendered_meshes(mjm, groups)
  if nbad:
    raise NotImplementedError(f"{nbad} visible mesh geom(s) of this model (geom group(s) {bad_groups}) have no triangles (Model.mesh_face: the loader "
                              "reads a mesh asset only for colliding or mass-carrying geoms): rays would silently pass through them; hide their group(s) with "
                              "enabled_geom_groups, or give those geoms rgba alpha 0, if that is meant")
  ncam = len(ids)
  if cam_res is None:
    res = [tuple(int(x) for x in cam.resolution[i]) for i in ids]
  elif len(cam_res) == 2 and all(isinstance(x, (int, np.integer)) for x in cam_res):
    res = [(int(cam_res[0]), int(cam_res[1]))] * ncam
  else:
    if len(cam_res) != ncam:
      raise ValueError(f"cam_res must be one (width, height) or one per active camera ({ncam}), got {len(cam_res)}")
    res = [(int(r[0]), int(r[1])) for r in cam_res]
  if any(w <= 0 or h <= 0 for w, h in res):
    raise ValueError(f"camera resolutions must be positive, got {res}")
  excl = [bool(exclude_camera_body)] * ncam if isinstance(exclude_camera_body, (bool, np.bool_)) else [bool(x) for x in exclude_camera_body]
  if len(excl) != ncam:
    raise ValueError(f"exclude_camera_body must be one bool or one per active camera ({ncam})")

  rc = RenderContext()
  rc.nworld, rc.ncam = int(nworld), ncam
  rc.cam_id = np.array(ids, dtype=np.int32)
  rc.cam_names = [cam.names[i] for i in ids]
  rc.cam_bodyid = cam.bodyid[ids].astype(np.int32)
  if ncam and (rc.cam_bodyid.min() < 0 or rc.cam_bodyid.max() >= mjm.nbody):
    raise ValueError("camera body id out of range")
  rc.cam_pos = cam.pos[ids].astype(np.float32).reshape(-1, 3)
  q = cam.quat[ids].reshape(-1, 4)
  rc.cam_quat = (q / np.maximum(np.linalg.norm(q, axis=1, keepdims=True), 1e-300)).astype(np.float32)
  rc.cam_fovy = cam.fovy[ids].astype(np.float32)
  rc.cam_res = np.array(res, dtype=np.int32).reshape(-1, 2)
  rc.cam_exclude = np.array([int(rc.cam_bodyid[k]) if excl[k] else -1 for k in range(ncam)], dtype=np.int32)
  npix = np.array([w * h for w, h in res], dtype=np.int64)
  adr = np.concatenate([[0], np.cumsum(npix)[:-1]]).astype(np.int64) if ncam else np.zeros(0, dtype=np.int64)
  rc.npixel = int(npix.sum())
  if rc.nworld * rc.npixel > 0x7FFFFFFF:
    raise ValueError(f"nworld * npixel = {rc.nworld * rc.npixel} exceeds 2^31 - 1: render fewer worlds or cameras per context")
  rc.depth_adr = adr.astype(np.int32)
  rc.seg_adr = adr.astype(np.int32)
  rc.znear = float(znear) if znear is not None else 0.01 * float(getattr(getattr(mjm, "stat", None), "extent", 1.0))
  if not rc.znear > 0.0:
    raise ValueError("znear must be positive")
  rc.ray = np.concatenate([compute_ray(float(cam.fovy[i]), w, h, rc.znear) for i, (w, h) in zip(ids, res)]).reshape(-1, 3) if ncam else np.zeros((0, 3), dtype=np.float32)
  rc.tile = np.array([(k, x, y) for k, (w, h) in enumerate(res) for y in range(0, h, TILE) for x in range(0, w, TILE)], dtype=np.int32).reshape(-1, 3)
  rc.enabled_geom_groups = tuple(groups)
  rc.groupmask = sum(1 << g for g in groups)
  rc.geomgroup = [1.0 if g in groups else 0.0 for g in range(6)]  # the same filter in rays()' form
  rc.render_depth, rc.render_seg, rc.render_normal = bool(render_depth), bool(render_seg), bool(render_normal)
  rc.depth_data = DeviceArray.zeros((rc.nworld, rc.npixel), np.float32) if render_depth else None
  rc.seg_data = DeviceArray.full((rc.nworld, rc.npixel, 2), -1, np.int32) if render_seg else None
  rc.normal_data = DeviceArray.zeros((rc.nworld, rc.npixel, 3), np.float32) if render_normal else None
  rc.cam_xpos = DeviceArray.zeros((rc.nworld, ncam, 3), np.float32)
  rc.cam_xmat = DeviceArray.zeros((rc.nworld, ncam, 9), np.float32)
  return rc


def _check_context(d, rc):
  if not isinstance(rc, RenderContext):
    raise TypeError("rc must be a RenderContext (create_render_context)")
  if rc.nworld != d.nworld:
    raise ValueError(f"the render context was built for nworld = {rc.nworld}, Data has {d.nworld}")


def render(m, d, rc: RenderContext):
  """Fill rc.cam_xpos / cam_xmat and the enabled outputs (depth_data, seg_data, normal_data) from d's current xpos / xmat / geom_xpos /
  geom_xmat (kinematics must have run).  Writes nothing into `d`."""
  _check_context(d, rc)
  if not (rc.render_depth or rc.render_seg or rc.render_normal):
    raise ValueError("the render context has no output enabled (render_depth, render_seg, render_normal)")
  _abi.check(_abi.lib().mjh_render(ctypes.byref(io.c_model(m)), ctypes.byref(io.c_data(d)), ctypes.byref(rc.c_render()), _stream()))


def camera_rays(m, d, rc: RenderContext, pnt_out: DeviceArray, vec_out: DeviceArray):
  """World-frame origin and direction [nworld, npixel, 3] of every pixel ray of `rc` (the rays render() casts; also refreshes
  rc.cam_xpos / cam_xmat): pass them to rays() with filters of your own."""
  _check_context(d, rc)
  for name, a in (("pnt_out", pnt_out), ("vec_out", vec_out)):
    if tuple(a.shape) != (d.nworld, rc.npixel, 3):
      raise ValueError(f"{name} must have shape ({d.nworld}, {rc.npixel}, 3), got {tuple(a.shape)}")
  _abi.check(_abi.lib().mjh_camera_rays(ctypes.byref(io.c_model(m)), ctypes.byref(io.c_data(d)), ctypes.byref(rc.c_render()), pnt_out.ptr, vec_out.ptr, _stream()))


def _camera_slice(rc, camera_index, out, trailing, what):
  if not 0 <= int(camera_index) < rc.ncam:
    raise ValueError(f"camera_index {camera_index} out of range (the context has {rc.ncam} active cameras)")
  w, h = (int(x) for x in rc.cam_res[camera_index])
  if tuple(out.shape) != (rc.nworld, h, w) + trailing:
    raise ValueError(f"{what} must have shape {(rc.nworld, h, w) + trailing} for camera {camera_index}, got {tuple(out.shape)}")
  return int(rc.depth_adr[camera_index]), w, h


def get_depth(rc: RenderContext, camera_index: int, depth_scale: float, depth_out: DeviceArray):
  """depth_out [nworld, height, width] = clamp(depth / depth_scale, 0, 1) of one camera (reference render_util.py:197)."""
  if rc.depth_data is None:
    raise ValueError("the render context was created with render_depth=False")
  adr, w, h = _camera_slice(rc, camera_index, depth_out, (), "depth_out")
  depth_out.t.copy_((rc.depth_data.t[:, adr:adr + w * h] / float(depth_scale)).clamp_(0.0, 1.0).reshape(rc.nworld, h, w))


def get_segmentation(rc: RenderContext, camera_index: int, seg_out: DeviceArray):
  """seg_out [nworld, height, width, 2] = (object id, object type) of one camera; background pixels are (-1, -1) (reference render_util.py:233)."""
  if rc.seg_data is None:
    raise ValueError("the render context was created with render_seg=False")
  adr, w, h = _camera_slice(rc, camera_index, seg_out, (2,), "seg_out")
  seg_out.t.copy_(rc.seg_data.t[:, adr:adr + w * h].reshape(rc.nworld, h, w, 2))
