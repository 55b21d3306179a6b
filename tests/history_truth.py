"""Float64 restatement of the actuator / sensor delay buffers: find / read / insert, the per-step protocol and the initial state.

Written from the description of the feature ("Delays") and the algorithm of the reference's history module, independently of
csrc/history.hpp: plain Python over numpy float64, one buffer at a time, no attempt at speed.

A buffer holds n samples (time, value[dim]) in a ring: `cursor` is the physical index of the newest sample, logical index i (0 = oldest)
lives at (cursor + 1 + i) % n, and times increase with the logical index.  In a row of Data.history a buffer is laid out as
[user, cursor, times[n], values[n * dim]].
"""

import numpy as np

EPS = 1e-6  # seconds: two times closer than this are the same sample
ZOH, LINEAR, CUBIC = 0, 1, 2


class Buffer:
  def __init__(self, n, dim=1):
    self.n, self.dim = int(n), int(dim)
    self.user = 0.0
    self.cursor = self.n - 1
    self.times = np.zeros(self.n)
    self.values = np.zeros((self.n, self.dim))

  # ---- layout -------------------------------------------------------------------------------------------------------------------
  @staticmethod
  def initial(n, dim, time, timestep):
    """The state make_data / reset_data give a buffer at `time`: zeros at time - (n - k) timestep, k = 0 .. n - 1, cursor n - 1, user 0."""
    b = Buffer(n, dim)
    b.times = time - (n - np.arange(n)) * float(timestep)
    return b

  @staticmethod
  def from_flat(row, adr, n, dim):
    """The buffer at `adr` of one world's row of Data.history."""
    b = Buffer(n, dim)
    row = np.asarray(row, dtype=np.float64)
    b.user, b.cursor = float(row[adr]), int(row[adr + 1])
    b.times = row[adr + 2 : adr + 2 + n].copy()
    b.values = row[adr + 2 + n : adr + 2 + n + n * dim].reshape(n, dim).copy()
    return b

  def flat(self):
    return np.concatenate([[self.user, float(self.cursor)], self.times, self.values.ravel()])

  def size(self):
    return 2 + self.n * (1 + self.dim)

  def copy(self):
    b = Buffer(self.n, self.dim)
    b.user, b.cursor, b.times, b.values = self.user, self.cursor, self.times.copy(), self.values.copy()
    return b

  # ---- ring ---------------------------------------------------------------------------------------------------------------------
  def phys(self, i):
    return (self.cursor + 1 + i) % self.n

  def logical_times(self):
    return np.array([self.times[self.phys(i)] for i in range(self.n)])

  def logical_values(self):
    return np.array([self.values[self.phys(i)] for i in range(self.n)])

  def find(self, t):
    """Smallest logical index i with time[i] >= t: 0 when t is not after the oldest sample, n when t is after the newest."""
    lt = self.logical_times()
    if t <= lt[0]:
      return 0
    if t > lt[-1]:
      return self.n
    lo, hi = 0, self.n - 1  # time[lo] < t <= time[hi]
    while hi - lo > 1:
      mid = (lo + hi) // 2
      if lt[mid] < t:
        lo = mid
      else:
        hi = mid
    return hi

  def read(self, t, interp):
    """The value at time t: clamped to the ends, an exact match within EPS as it is, else interpolated component by component."""
    lt, lv = self.logical_times(), self.logical_values()
    if t <= lt[0] + EPS:
      return lv[0].copy()
    if t >= lt[-1] - EPS:
      return lv[-1].copy()
    i = self.find(t)
    if abs(t - lt[i]) < EPS:
      return lv[i].copy()
    if interp == ZOH:
      return lv[i - 1].copy()
    dt = lt[i] - lt[i - 1]
    a = (t - lt[i - 1]) / dt
    if interp == LINEAR:
      return lv[i - 1] + a * (lv[i] - lv[i - 1])
    # cubic Hermite, Catmull-Rom slopes from the neighbours, zero slope where the buffer ends
    m_lo = (lv[i] - lv[i - 2]) / (lt[i] - lt[i - 2]) if i > 1 else np.zeros(self.dim)
    m_hi = (lv[i + 1] - lv[i - 1]) / (lt[i + 1] - lt[i - 1]) if i < self.n - 1 else np.zeros(self.dim)
    a2, a3 = a * a, a * a * a
    return (2 * a3 - 3 * a2 + 1) * lv[i - 1] + (a3 - 2 * a2 + a) * dt * m_lo + (-2 * a3 + 3 * a2) * lv[i] + (a3 - a2) * dt * m_hi

  def insert(self, t, value):
    """Exact match: overwrite; older than the oldest: replace the oldest; newer than the newest: advance the cursor; else shift the older
    samples down by one (the oldest goes) and insert."""
    value = np.asarray(value, dtype=np.float64).reshape(self.dim)
    i = self.find(t)
    if i < self.n and abs(t - self.times[self.phys(i)]) < EPS:
      self.values[self.phys(i)] = value
      return
    if i == 0:
      p = self.phys(0)
    elif i == self.n:
      self.cursor = (self.cursor + 1) % self.n
      p = self.cursor
    else:
      for j in range(i - 1):
        self.times[self.phys(j)] = self.times[self.phys(j + 1)]
        self.values[self.phys(j)] = self.values[self.phys(j + 1)]
      p = self.phys(i - 1)
    self.times[p] = t
    self.values[p] = value


# ---- the protocol of one forward evaluation / step ---------------------------------------------------------------------------------
def evaluate(buf, t, delay, interp, fresh, insert):
  """What an actuator (fresh = ctrl) or a sensor (fresh = its computed values) with the buffer `buf` contributes to an evaluation at time t:
  the buffer read at t - delay when it has a delay, the fresh values otherwise; the read comes first, then -- when asked -- the fresh
  values are inserted at t.  buf None: no buffer, the fresh values pass."""
  fresh = np.atleast_1d(np.asarray(fresh, dtype=np.float64))
  if buf is None:
    return fresh.copy()
  out = buf.read(t - delay, interp) if delay > 0 else fresh.copy()
  if insert:
    buf.insert(t, fresh)
  return out
