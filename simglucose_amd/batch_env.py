"""BatchedT1DSimEnv: N independent T1DSimEnv episodes advanced by one HIP kernel launch per step.

The host side holds the batched state as struct-of-arrays PyTorch-ROCm tensors (env index fastest)
and hands their device pointers to libt1d_hip.so through the C ABI of include/t1d.h.  Semantics per
env are those of the reference's ``simglucose/simulation/env.py`` ``T1DSimEnv.reset/step`` composed
of ``T1DPatient`` + ``CGMSensor`` + ``InsulinPump`` + a meal scenario; instead of SciPy's adaptive DOPRI5 the ODE is
integrated by the library's split scheme built on ``n_sub`` sub-steps per minute, with per-minute step sizes chosen by a
deterministic rule (``adaptive_gut``), or by classical RK4 (``set_option("integrator", 0)``).
``integrator="dopri5"`` runs SciPy's DOPRI5 itself as the reference drives it (t1d_step_dopri5): the reference's numbers,
at a few times the cost.  Closed-loop roll-outs in that mode are ``rollout_pid_dopri5`` / ``rollout_bb_dopri5``
(t1d_rollout_pid_dopri5 / t1d_rollout_bb_dopri5): every env walks through its minutes at its own pace inside a launch, with
the results of a ``step()`` loop bit for bit.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib, params

_STATE_KEYS = ("x", "planned", "last_qsto", "last_food", "t", "meta", "episode", "next_meal", "last_cgm", "ar_e",
               "pts", "prev_risk", "dbar")
_OUT_KEYS = ("cgm", "bg", "reward", "done", "lbgi", "hbgi", "risk", "meal", "insulin", "cgm0")


class BatchedT1DSimEnv:
    """A batch of ``n`` glucose-insulin simulation environments on one MI355X.

    patient: one name, a list of names (len n) or an integer array of table rows (len n).
    sensor / pump: hardware names from the parameter tables (one per batch).
    noise: "philox" draws the CGM noise normals in-kernel (rocRAND Philox4x32-10, stream =
           global env id); "host" reads them from ``normals[n_draws, n]`` (exact parity with
           ``numpy.random.RandomState(seed).randn()`` streams supplied by the caller).
    cgm_history: keep the last hour of observations per env on the device -- the ``CGM_hist[-window:]`` that
           ``T1DSimEnv.step`` hands to a custom ``reward_fun`` (simulation/env.py:100-102), window = 60 / sample_time
           samples -- so that ``step(..., reward_fun=f)`` works on the batch: ``f(window)`` gets a ``[window, n]``
           tensor, oldest sample first, NaN where an episode is younger than that, and returns ``[n]`` rewards.
           Off by default: the fused default reward (risk_diff) needs only the previous sample.
    integrator: None = the library's fixed-step schemes (above); "dopri5" = the exact mode, scipy's dopri5 with the
           reference's tolerances re-entered every minute (t1d_step_dopri5; fp64 only, n_sub ignored).  The predicted step of
           each env is kept in ``h_carry`` (fp64 [n], zeroed by reset) and the RHS evaluations of the last step in ``nfev``
           (int32 [n]).  Closed-loop roll-outs of such an env: ``rollout_pid_dopri5`` / ``rollout_bb_dopri5`` (same arguments and
           results as ``rollout_pid`` / ``rollout_bb``, which take the fixed-step envs only); ``nfev`` then holds the RHS
           evaluations of the whole call.
    """

    def __init__(self, patient="adolescent#001", n_envs=None, sensor="Dexcom", pump="Insulet",
                 dtype=torch.float64, device="cuda:0", n_sub=4, seed=0, env_offset=0, noise="philox",
                 normals=None, random_init_bg=False, extra_outputs=True, sensor_row=None, pump_row=None,
                 patient_table=None, use_pump=True, adaptive_gut=True, cgm_history=False, integrator=None):
        if integrator not in (None, "dopri5"):
            raise ValueError("integrator must be None or 'dopri5'")
        if integrator == "dopri5" and dtype != torch.float64:
            raise ValueError("integrator='dopri5' needs dtype=torch.float64")
        self.integrator = integrator
        self._L = _lib.lib()                     # raises T1DError if the HIP extension is missing
        if not torch.cuda.is_available():
            raise _lib.T1DError("BatchedT1DSimEnv needs a ROCm GPU (torch.cuda.is_available() is False)")
        if dtype not in (torch.float64, torch.float32):
            raise ValueError("dtype must be torch.float64 or torch.float32")
        self.device = torch.device(device)
        self.dtype = dtype
        self.n_sub = int(n_sub)
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.env_offset = int(env_offset)
        self.random_init_bg = bool(random_init_bg)
        self.names, self.table = params.patient_table()
        if patient_table is not None:            # caller-supplied rows (T1D_P_* column order), e.g. edited parameters
            self.table = np.ascontiguousarray(np.atleast_2d(np.asarray(patient_table, dtype=np.float64)))
            if self.table.shape[1] != _lib.P_NCOLS:
                raise ValueError("patient_table must have %d columns" % _lib.P_NCOLS)
            self.names = ["custom#%03d" % k for k in range(self.table.shape[0])]
        if isinstance(patient, str) and patient_table is not None:
            patient = np.zeros(int(n_envs or 1), dtype=np.int64)
        if isinstance(patient, str):
            if n_envs is None:
                n_envs = 1
            pid = np.full(int(n_envs), params.patient_index(patient), dtype=np.int64)
        else:
            arr = list(patient) if not isinstance(patient, (np.ndarray, torch.Tensor)) else patient
            if len(arr) and isinstance(arr[0], str):
                pid = np.array([params.patient_index(p) for p in arr], dtype=np.int64)
            else:
                pid = np.asarray(torch.as_tensor(arr).cpu().numpy(), dtype=np.int64)
            if n_envs is not None and int(n_envs) != len(pid):
                raise ValueError("n_envs does not match the patient list")
        if pid.size < 1 or pid.min() < 0 or pid.max() >= len(self.names):
            raise ValueError("patient index out of range")
        self.n = int(pid.size)
        self.patient_idx = pid
        self.sensor_name, self.pump_name = sensor, pump
        self.sensor_row = np.asarray(sensor_row if sensor_row is not None else params.sensor_row(sensor), dtype=np.float64)
        self.pump_row = np.asarray(pump_row if pump_row is not None else params.pump_row(pump), dtype=np.float64)
        self.sample_time = float(self.sensor_row[5])
        self.minutes_per_step = int(self.sample_time)

        dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self._ctx = C.c_void_p()
        dp = C.POINTER(C.c_double)
        tab = np.ascontiguousarray(self.table)
        _lib.check(self._L.t1d_ctx_create(dev_index, tab.ctypes.data_as(dp), tab.shape[0], tab.shape[1],
                                          self.sensor_row.ctypes.data_as(dp), self.pump_row.ctypes.data_as(dp),
                                          C.byref(self._ctx)))
        # split integrator: half-size gut steps in the minutes that cross a gastric-emptying transition fast (library default)
        self.set_option("adaptive_gut", 1 if adaptive_gut else 0)
        n, dv, ft = self.n, self.device, dtype
        z = lambda *shape, dt=ft: torch.zeros(*shape, dtype=dt, device=dv)
        # packed state (include/t1d.h): one [45, n] float buffer and one [4, n] int32 buffer; the named
        # tensors are views, so every staged row is one base pointer plus a 32-bit offset on the device
        self.state = z(45, n)
        self.x = self.state[0:13]; self.planned = self.state[13]; self.last_qsto = self.state[14]
        self.last_food = self.state[15]; self.last_cgm = self.state[16]; self.prev_risk = self.state[17]
        self.pts = self.state[18:44]; self.dbar = self.state[44]
        self.istate = z(4, n, dt=torch.int32)
        self.t = self.istate[0]; self.meta = self.istate[1]; self.next_meal = self.istate[2]; self.episode = self.istate[3]
        self.meta.copy_(torch.from_numpy(pid.astype(np.int32)))            # patient row in bits 0-7
        self.next_meal.fill_(_lib.MEAL_UNUSED)
        self.ar_e = z(n)
        self.cgm = z(n); self.bg = z(n); self.reward = z(n); self.done = z(n, dt=torch.uint8)
        self.cgm0 = z(n)                   # CGM sample #0 of the current episode (CGM_hist[0]); written by reset only
        if extra_outputs:
            self.lbgi = z(n); self.hbgi = z(n); self.risk = z(n); self.meal = z(n); self.insulin = z(n)
        else:
            self.lbgi = self.hbgi = self.risk = self.meal = self.insulin = None
        self._zero_action = z(n)
        if integrator == "dopri5":
            self.h_carry = z(n, dt=torch.float64)          # predicted step per env; 0 = probe for one (after reset)
            self.nfev = z(n, dt=torch.int32)               # RHS evaluations per env in the last step
        else:
            self.h_carry = self.nfev = None
        self._basal_buf = z(n); self._bolus_buf = z(n)
        self.meal_time = None; self.meal_amt = None
        self.start_minute = None   # int32 [n], minute of day at which each env's current episode started (restart_done)
        self.normals = None
        self._b = _lib.Batch()
        b = self._b
        b.n, b.env_offset, b.dtype, b.seed = n, self.env_offset, (_lib.T1D_F64 if ft == torch.float64 else _lib.T1D_F32), self.seed
        for k in _STATE_KEYS + _OUT_KEYS:
            tns = getattr(self, k)
            setattr(b, k, tns.data_ptr() if tns is not None else None)
        b.n_meals = 0; b.n_normals = 0
        b.flags = 0 if use_pump else _lib.T1D_BATCH_NO_PUMP
        if noise not in ("philox", "host"):
            raise ValueError("noise must be 'philox' or 'host'")
        self.noise = noise
        if noise == "host":
            if normals is None:
                raise ValueError("noise='host' needs normals[n_draws, n]")
            self.set_normals(normals)
        self._closed = False
        self._clock = None         # minutes since the last FULL reset while every env shares one clock, else None
        self._iver = None          # version counter of the integer state tensors when the shadow clock was last valid
        self._flags0 = b.flags
        self.window = int(60 / self.sample_time)            # samples a custom reward function sees (env.py:100)
        self._hist = self._hist_pos = self._hist_cnt = None
        if cgm_history:
            self.enable_cgm_history()

    # ------------------------------------------------------------------ inputs
    def _as_input(self, v, buf):
        """-> a contiguous [n] tensor of the env dtype on the env device (copying only if needed)."""
        if isinstance(v, torch.Tensor) and v.dtype == self.dtype and v.device == self.device and v.shape == (self.n,) \
                and v.is_contiguous():
            return v
        buf.copy_(torch.as_tensor(v, dtype=self.dtype, device=self.device).expand(self.n))
        return buf

    def set_normals(self, normals):
        """Host-supplied standard normals [n_draws, n]: row 0 seeds the AR(1) state, rows 1.. are
        consumed ten per 150-minute noise block (noise_gen.py:84-97)."""
        t = torch.as_tensor(normals, dtype=self.dtype).to(self.device).contiguous()
        if t.dim() != 2 or t.shape[1] != self.n:
            raise ValueError("normals must have shape [n_draws, n]")
        self.normals = t
        self._b.normals = t.data_ptr(); self._b.n_normals = t.shape[0]
        self.noise = "host"

    def set_meals(self, meal_time, meal_amt):
        """Per-env meal table: meal_time[m, i] = minute since episode start (ascending per env,
        unused = MEAL_UNUSED), meal_amt[m, i] = grams announced at that minute."""
        mt = torch.as_tensor(meal_time).to(torch.int32).to(self.device).contiguous()
        ma = torch.as_tensor(meal_amt).to(self.dtype).to(self.device).contiguous()
        if mt.dim() != 2 or mt.shape != ma.shape or mt.shape[1] != self.n:
            raise ValueError("meal tables must both have shape [n_meals, n]")
        self.meal_time, self.meal_amt = mt, ma
        self._b.meal_time, self._b.meal_amt, self._b.n_meals = mt.data_ptr(), ma.data_ptr(), mt.shape[0]
        # restart the table scan: cursor 0, next entry = row 0 (rows before the current minute are skipped lazily)
        self.meta.bitwise_and_(0xFFFF)
        self.next_meal.copy_(mt[0])

    def set_option(self, name, value):
        """t1d_ctx_set_option (include/t1d.h): e.g. ("integrator", 0) = classical RK4, ("adaptive_gut", 0) = the split
        scheme at level 1 in every minute, ("math", 0) = the ocml-tanh / IEEE-division RHS with classical RK4."""
        _lib.check(self._L.t1d_ctx_set_option(self._ctx, name.encode(), int(value)))

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    # ------------------------------------------------------------------ CGM history for custom reward functions
    def enable_cgm_history(self):
        """allocate the per-env ring of the last `window` observations (call before reset())"""
        if self._hist is None:
            self._hist = torch.full((self.window, self.n), float("nan"), dtype=self.dtype, device=self.device)
            self._hist_pos = torch.zeros(self.n, dtype=torch.int64, device=self.device)
            self._hist_cnt = torch.zeros(self.n, dtype=torch.int64, device=self.device)

    def _hist_reset(self, mask):
        """T1DSimEnv._reset: CGM_hist = [sample #0] (env.py:126), which the reset kernel leaves in cgm0"""
        if self._hist is None:
            return
        m = torch.ones(self.n, dtype=torch.bool, device=self.device) if mask is None else mask.bool()
        self._hist[:, m] = float("nan")
        self._hist_pos[m] = 0
        self._hist_cnt[m] = 1
        self._hist[0, m] = self.cgm0[m]

    def _hist_restart(self, m):
        """_hist_reset for the envs of the bool mask m without boolean indexing (nothing here waits for the device)"""
        if self._hist is None:
            return
        nan = torch.full((), float("nan"), dtype=self.dtype, device=self.device)
        self._hist.copy_(torch.where(m.unsqueeze(0), nan, self._hist))
        self._hist[0].copy_(torch.where(m, self.cgm0, self._hist[0]))
        self._hist_pos.masked_fill_(m, 0)
        self._hist_cnt.masked_fill_(m, 1)

    def _hist_push(self):
        """CGM_hist.append(CGM) (env.py:94) for every env"""
        self._hist_pos = (self._hist_pos + 1) % self.window
        self._hist.scatter_(0, self._hist_pos.unsqueeze(0), self.cgm.unsqueeze(0))
        self._hist_cnt = torch.clamp(self._hist_cnt + 1, max=self.window)

    def _hist_after_rollout(self):
        """a roll-out advances many steps inside one launch: what the ring holds afterwards is the last observation only"""
        if self._hist is not None:
            self._hist.fill_(float("nan"))
            self._hist_pos.zero_()
            self._hist_cnt.fill_(1)
            self._hist[0] = self.cgm

    def cgm_window(self):
        """-> [window, n]: CGM_hist[-window:] of every env, oldest first, NaN-padded at the top while an episode has fewer
        samples (the reference passes a shorter list then)."""
        if self._hist is None:
            raise _lib.T1DError("the CGM history is off: construct with cgm_history=True (or call enable_cgm_history() before reset())")
        k = torch.arange(self.window, device=self.device).unsqueeze(1)
        w = torch.gather(self._hist, 0, (self._hist_pos.unsqueeze(0) + 1 + k) % self.window)
        return torch.where(k >= self.window - self._hist_cnt.unsqueeze(0), w, torch.full_like(w, float("nan")))

    # ------------------------------------------------------------------ reset / step
    def reset(self, mask=None, x0=None):
        """T1DSimEnv.reset() on every env (or those with mask != 0).  -> observation CGM [n]."""
        b = self._b
        keep = None
        if x0 is not None:
            keep = torch.as_tensor(x0, dtype=self.dtype).to(self.device).contiguous()
            if keep.shape != (13, self.n):
                raise ValueError("x0 must have shape [13, n]")
            b.x0_override = keep.data_ptr()
        else:
            b.x0_override = None
        mptr = None
        if mask is not None:
            mask = torch.as_tensor(mask).to(self.device).to(torch.uint8).contiguous()
            mptr = C.c_void_p(mask.data_ptr())
        self._clock = 0 if mask is None else None
        with torch.cuda.device(self.device):
            _lib.check(self._L.t1d_reset(self._ctx, C.byref(b), mptr, int(self.random_init_bg), self._stream()))
        if self.h_carry is not None:                      # scipy's solver is built afresh by T1DPatient.reset
            if mask is None:
                self.h_carry.zero_()
            else:
                self.h_carry.masked_fill_(mask.bool(), 0.0)
        self._iver = self.istate._version
        b.x0_override = None
        self._keep = (keep, mask)
        self._hist_reset(mask)
        return self.cgm

    def restart_done(self, mask=None, days=2, terminal_obs=None, episode_stats=None, reset_outputs=False):
        """Start the next episode of the finished envs where they are (t1d_restart_done, include/t1d.h): one launch after a
        step(), no host round trip.  mask: uint8 / bool [n], None = ``done``.  A restarted env draws its start hour, its column
        of the meal tables (RandomScenario over ``days`` days) and its reset from its own episode index (``episode`` before the
        call) and global id, so its k-th episode does not depend on the rest of the batch.  Of the outputs only ``cgm`` (the new
        episode's first observation) changes; reward, done, bg ... keep the terminal step's values unless reset_outputs.
        The env owns meal tables of 6 (days + 1) rows (created on the first call if it has none) and ``start_minute``.
        terminal_obs: tensor [n] that receives the finished step's observation of the restarted envs.  episode_stats: dict
        with ep_return, ep_length (int32) and optionally last_return, last_length (int32), tensors [n]: every call adds the
        step's reward and 1 to the running pair, a restart moves it to last_* and zeroes it."""
        if self.noise == "host" or self.normals is not None:
            raise _lib.T1DError("restart_done draws every episode on the device: not available with host normals")
        r = self._restart_struct(int(days), terminal_obs, episode_stats or {}, reset_outputs, "restart_done")
        st = episode_stats or {}
        mptr = None
        if mask is not None:
            mask = torch.as_tensor(mask)
            if mask.dtype == torch.bool and mask.device == self.device and mask.is_contiguous():
                mask = mask.view(torch.uint8)
            else:
                mask = mask.to(self.device).to(torch.uint8).contiguous()
            if mask.shape != (self.n,):
                raise ValueError("mask must have n entries")
            mptr = C.c_void_p(mask.data_ptr())
        self._b.x0_override = None
        self._clock = None                         # the envs no longer share one clock
        # the ring is reset from the mask as it is before the launch (reset_outputs clears `done`)
        hist_mask = None if self._hist is None else (self.done if mask is None else mask).bool()
        with torch.cuda.device(self.device):
            _lib.check(self._L.t1d_restart_done(self._ctx, C.byref(self._b), mptr, C.byref(r), self._stream()))
        self._keep = (mask, terminal_obs, st)
        if hist_mask is not None:
            self._hist_restart(hist_mask)
        return self.cgm

    def _restart_struct(self, days, terminal_obs, st, reset_outputs, who):
        """the t1d_restart of restart_done / collect_mlp; creates the env's meal tables and start_minute if it has none"""
        rows = 6 * (days + 1)
        if self.meal_time is None:
            self.set_meals(torch.full((rows, self.n), _lib.MEAL_UNUSED, dtype=torch.int32, device=self.device),
                           torch.zeros(rows, self.n, dtype=self.dtype, device=self.device))
        if self.meal_time.shape[0] != rows:
            raise _lib.T1DError("%s(days=%d) needs meal tables of %d rows; the env's have %d"
                                % (who, days, rows, self.meal_time.shape[0]))
        if self.start_minute is None:
            self.start_minute = torch.zeros(self.n, dtype=torch.int32, device=self.device)
        r = _lib.Restart()
        r.days, r.random_init_bg, r.reset_outputs, r.reserved = days, int(self.random_init_bg), int(bool(reset_outputs)), 0
        r.meal_time, r.meal_amt = self.meal_time.data_ptr(), self.meal_amt.data_ptr()
        r.start_minute = self.start_minute.data_ptr()
        r.h_carry = self.h_carry.data_ptr() if self.h_carry is not None else None

        def ptr(t, dt):
            if t is None:
                return None
            if t.dtype != dt or t.device != self.device or t.shape != (self.n,) or not t.is_contiguous():
                raise ValueError("%s buffers must be contiguous [n] tensors of %s on the env's device" % (who, dt))
            return t.data_ptr()
        r.terminal_cgm = ptr(terminal_obs, self.dtype)
        r.ep_return, r.ep_length = ptr(st.get("ep_return"), self.dtype), ptr(st.get("ep_length"), torch.int32)
        r.last_return, r.last_length = ptr(st.get("last_return"), self.dtype), ptr(st.get("last_length"), torch.int32)
        return r

    def step(self, basal, bolus=None, cho=None, minutes=None, reward_fun=None):
        """One env.step for the whole batch: a single kernel launch advancing ``minutes``
        (default int(sample_time)) with the action held.  -> (obs CGM [n], reward [n], done [n], info).
        reward_fun: None = the fused default, risk_diff (env.py:27-33); a callable gets ``cgm_window()`` -- the batch
        form of ``reward_fun(CGM_hist[-window:])``, env.py:100-102 -- and returns the rewards [n] (needs cgm_history)."""
        b = self._b
        minutes = self.minutes_per_step if minutes is None else int(minutes)
        bas = self._as_input(basal, self._basal_buf)
        b.basal = bas.data_ptr()
        if bolus is None:
            b.bolus = None
        else:
            b.bolus = self._as_input(bolus, self._bolus_buf).data_ptr()
        if cho is not None:
            cho = torch.as_tensor(cho, dtype=self.dtype).to(self.device).contiguous()
            if cho.shape != (minutes, self.n):
                raise ValueError("cho must have shape [minutes, n]")
            b.cho = cho.data_ptr()
        else:
            b.cho = None
        b.flags = self._flags0
        if self._clock is not None and self.istate._version != self._iver:
            # somebody wrote env.t / env.meta / env.next_meal through torch since the shadow clock was taken (kernel
            # launches do not move the version counter): the envs' own clocks decide again
            self._clock = None
        if self._clock is not None:
            # every env shares the clock: the host knows whether a sample in (t, t + minutes] opens a noise block
            st, S = self.minutes_per_step, int(150 // self.sample_time)
            due = any((t1 % st == 0) and ((1 + t1 // st) % S == 0) for t1 in range(self._clock + 1, self._clock + minutes + 1))
            if not due:
                b.flags = self._flags0 | _lib.T1D_BATCH_NO_REFILL_DUE
        clock, self._clock = self._clock, None        # the shadow clock survives only a call that went through
        with torch.cuda.device(self.device):
            if self.integrator == "dopri5":
                _lib.check(self._L.t1d_step_dopri5(self._ctx, C.byref(b), C.c_void_p(self.h_carry.data_ptr()),
                                                   C.c_void_p(self.nfev.data_ptr()), minutes, self._stream()))
            else:
                _lib.check(self._L.t1d_step(self._ctx, C.byref(b), minutes, self.n_sub, self._stream()))
        if clock is not None:
            self._clock = clock + minutes
        self._keep = (bas, cho)
        if self._hist is not None:
            self._hist_push()
        if reward_fun is not None:
            reward = torch.as_tensor(reward_fun(self.cgm_window()), dtype=self.dtype, device=self.device).expand(self.n)
            return self.cgm, reward, self.done, self.info()
        return self.cgm, self.reward, self.done, self.info()

    def info(self):
        """live views of the device outputs and state: read-only for the caller (the reference's info['patient_state']
        is the solver's own array too, env.py:112).  The wrapper shadows the clock on the host to skip the noise-block
        refill pre-kernel; an in-place torch edit of env.t / env.meta / env.next_meal is noticed (the tensors' version
        counter) and drops the shadow, so that such an edit cannot leave a stale noise block behind -- for writes the
        counter cannot see there is invalidate_clock().  (A copy of t per step would cost a 4 MB device copy per launch at
        1 Mi envs: 6 % of the step.)"""
        return {"sample_time": self.sample_time, "bg": self.bg, "lbgi": self.lbgi, "hbgi": self.hbgi,
                "risk": self.risk, "meal": self.meal, "insulin": self.insulin, "patient_state": self.x,
                "t": self.t}

    def invalidate_clock(self):
        """forget the host's shadow clock: the next steps check every env's own clock for due noise-block refills again.
        (In-place torch edits of env.t / env.meta / env.next_meal are noticed through the tensors' version counter; this
        is for writes the counter cannot see, e.g. through a raw pointer.)"""
        self._clock = None

    @staticmethod
    def _set_trace(p, trace, n_steps):
        """trace: None or dict with any of bg, cgm, cho, insulin (tensors [rows, n]) and row = first row to write
        (see new_trace); rollout_mlp also takes action"""
        p.bg_trace = p.cgm_trace = p.cho_trace = p.insulin_trace = None
        p.trace_row = 0
        cols = (("bg", "bg_trace"), ("cgm", "cgm_trace"), ("cho", "cho_trace"), ("insulin", "insulin_trace"))
        if hasattr(p, "action_trace"):
            p.action_trace = None
            cols += (("action", "action_trace"),)
        if trace:
            row = int(trace.get("row", 0))
            for k, f in cols:
                if trace.get(k) is not None:
                    if trace[k].shape[0] < row + n_steps or not trace[k].is_contiguous():
                        raise ValueError("trace['%s'] needs at least row + n_steps contiguous rows" % k)
                    setattr(p, f, trace[k].data_ptr())
            p.trace_row = row
            trace["row"] = row + int(n_steps)

    def new_trace(self, n_steps, columns=("bg", "cgm", "cho", "insulin"), history=None):
        """Device-resident history for the next `n_steps` roll-out steps, laid out as T1DSimEnv's history lists
        (simulation/env.py:119-155,169-180): row 0 holds what reset() recorded (BG0 and CGM sample #0; CHO and
        insulin have no row for the last time stamp, so their row r is the action of step r), row r >= 1 step r.
        "action" (rollout_mlp, collect_mlp) is the basal the policy asked for in step r, before the pump; "bolus" (a policy
        with meal_bolus) the meal bolus of step r, before the pump.
        collect_mlp only: "reward", "done" (uint8) and "eps" of step r, and "features" [n_steps + 1, F, n], what the
        network was given in step r (F = 2 history + 3: pass the policy's history=); their row 0 is NaN (0 for "done").
        "truncated" (uint8, collect_mlp_limit and the other *_limit collectors): 1 where step r was cut by the time limit; row 0 is 0.
        Call right after reset(); pass the dict as rollout_*(trace=...)."""
        tr = {"row": 1}
        for k in columns:
            if k in ("done", "truncated"):
                tr[k] = torch.zeros(int(n_steps) + 1, self.n, dtype=torch.uint8, device=self.device)
                continue
            shape = (int(n_steps) + 1, self.n)
            if k == "features":
                if history is None:
                    raise ValueError("new_trace: the 'features' column needs history= (the policy's window length)")
                shape = (int(n_steps) + 1, 2 * int(history) + 3, self.n)
            tr[k] = torch.full(shape, float("nan"), dtype=self.dtype, device=self.device)
        if "bg" in tr:
            tr["bg"][0] = self.bg
        if "cgm" in tr:
            tr["cgm"][0] = self.cgm0
        return tr

    def _no_dopri5_rollout(self):
        if self.integrator == "dopri5":
            raise _lib.T1DError("rollout_pid / rollout_bb / rollout_mlp / collect_mlp / collect_pid / collect_bb run the fixed-step "
                                "kernels, which have no DOPRI5 path: an env with integrator='dopri5' takes rollout_pid_dopri5 / "
                                "rollout_bb_dopri5 / rollout_mlp_dopri5 / collect_mlp_dopri5 (collect_pid and collect_bb have no "
                                "exact-mode form in these kernels: collect_pid_dopri5 / collect_bb_dopri5)")

    def rollout_pid(self, n_steps, P, I=None, D=None, target=140.0, pid_state=None, stats=None, trace=None):
        """n_steps closed-loop PID steps in one launch (PIDController.policy + env.step per step).
        pid_state: dict(integ, prev) tensors [n] (created zeroed if None).  stats: optional dict
        with any of sum_risk, min_bg, max_bg (float [n]) and n_low, n_high (int32 [n]).
        P, I, D, target: four numbers, one controller for every env (t1d_rollout_pid) -- or, any of them a tensor or array of
        n numbers, or P the dict pid_gains() returns (I and D then left out), a controller per env (t1d_rollout_pid_gains):
        env i runs under P[i], I[i], D[i], target[i] and is, bit for bit, the env of a batch run entirely under those four
        numbers, so a grid of gain sets x patients x scenarios is one batch and one roll-out."""
        self._no_dopri5_rollout()
        gains = self._per_env_gains("rollout_pid", P, I, D, target)
        if gains is None:
            pid_state, p = self._pid_struct(P, I, D, target, pid_state, stats)
            self._rollout(self._L.t1d_rollout_pid, (p,), n_steps, trace)
        else:
            pid_state, p = self._pid_struct(0.0, 0.0, 0.0, 0.0, pid_state, stats)
            self._rollout(self._L.t1d_rollout_pid_gains, (p, self._gains_struct(gains)), n_steps, trace)
        return pid_state

    _GAIN_NAMES = ("P", "I", "D", "target")

    @staticmethod
    def _is_per_env(v):
        """a gain given per env: anything with a length or a shape, i.e. not a plain number"""
        return isinstance(v, (torch.Tensor, np.ndarray, list, tuple))

    def pid_gains(self, P, I, D, target=140.0):
        """The four [n] arrays of a per-env PID controller, as rollout_pid / rollout_pid_dopri5 take them in place of four
        numbers: dict(P, I, D, target) of contiguous tensors in the env's dtype on its device.  A number is broadcast; a
        tensor or array of n numbers is taken in float64 and rounded once to the env's dtype (what the scalar call does
        with its doubles); any other length is a ValueError.  A tensor that already is [n], contiguous, of the env's
        dtype and on its device is used in place: the caller may edit it between roll-outs."""
        out = {}
        for name, v in zip(self._GAIN_NAMES, (P, I, D, target)):
            if isinstance(v, torch.Tensor) and v.shape == (self.n,) and v.dtype == self.dtype and v.device == self.device and v.is_contiguous():
                out[name] = v
                continue
            if self._is_per_env(v):
                w = v.detach().to("cpu", torch.float64) if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v, dtype=np.float64))
                if w.dim() == 0:
                    w = w.reshape(1).expand(self.n)
                elif tuple(w.shape) != (self.n,):
                    raise ValueError("pid_gains: %s has shape %s, the env has %d envs (one number, or [%d])"
                                     % (name, tuple(w.shape), self.n, self.n))
            else:
                w = torch.full((self.n,), float(v), dtype=torch.float64)
            out[name] = w.to(self.dtype).to(self.device).contiguous()
        return out

    def _per_env_gains(self, who, P, I, D, target):
        """None where the four are plain numbers (the scalar entry point); else the dict of pid_gains, checked"""
        if isinstance(P, dict):
            if I is not None or D is not None:
                raise ValueError("%s: with the dict of pid_gains() as P, leave I and D out" % who)
            missing = [k for k in self._GAIN_NAMES if k not in P]
            if missing:
                raise ValueError("%s: the gains dict has no %s (see pid_gains)" % (who, ", ".join(missing)))
            return self.pid_gains(P["P"], P["I"], P["D"], P["target"])
        if I is None or D is None:
            raise TypeError("%s needs P, I and D (or the dict of pid_gains() as P)" % who)
        if not any(self._is_per_env(v) for v in (P, I, D, target)):
            return None
        return self.pid_gains(P, I, D, target)

    def _gains_struct(self, gains):
        g = _lib.PidGains()
        g.P, g.I, g.D, g.target = (gains[k].data_ptr() for k in self._GAIN_NAMES)
        self._keep_gains = gains                       # the arrays outlive the launch
        return g

    def _no_per_env_gains(self, who, *gains):
        if any(isinstance(v, dict) or self._is_per_env(v) for v in gains):
            raise _lib.T1DError("%s takes one P, I, D and target for the whole batch: per-env gains are a roll-out feature "
                                "(rollout_pid / rollout_pid_dopri5 take tensors or the dict of pid_gains())" % who)

    @staticmethod
    def _n_steps(n_steps):
        n_steps = int(n_steps)
        if n_steps < 1:
            raise ValueError("n_steps must be at least 1")
        return n_steps

    @staticmethod
    def _set_stats(p, stats):
        """stats: None or dict with any of the five accumulators -> the fields of a t1d_pid / t1d_bb / t1d_mlp"""
        stats = stats or {}
        for k in ("sum_risk", "min_bg", "max_bg", "n_low", "n_high"):
            setattr(p, k, stats[k].data_ptr() if k in stats else None)

    def _pid_struct(self, P, I, D, target, pid_state, stats):
        """the t1d_pid of rollout_pid / rollout_pid_dopri5 / collect_pid -> (pid_state, created zeroed if None; struct)"""
        if pid_state is None:
            pid_state = {"integ": torch.zeros(self.n, dtype=self.dtype, device=self.device),
                         "prev": torch.zeros(self.n, dtype=self.dtype, device=self.device)}
        p = _lib.Pid()
        p.P, p.I, p.D, p.target = float(P), float(I), float(D), float(target)
        p.integ, p.prev = pid_state["integ"].data_ptr(), pid_state["prev"].data_ptr()
        self._set_stats(p, stats)
        return pid_state, p

    def _bb_struct(self, target, bb_state, stats):
        """the t1d_bb of rollout_bb / rollout_bb_dopri5 / collect_bb -> (bb_state, created from bb_constants() if None; struct)"""
        if bb_state is None:
            bb_state = self.bb_constants()
            bb_state["prev_meal"] = torch.zeros(self.n, dtype=self.dtype, device=self.device)
        p = _lib.Bb()
        p.target = float(target)
        for k in ("basal", "cr", "cf", "prev_meal"):
            setattr(p, k, bb_state[k].data_ptr())
        self._set_stats(p, stats)
        return bb_state, p

    def _rollout(self, fn, structs, n_steps, trace, restarts=False):
        """The one fixed-step closed-loop launch: fn(ctx, batch, *structs, n_steps, minutes, n_sub, stream).  structs[0] is
        the controller's, which carries the trace columns of _set_trace; a struct that is None goes as NULL.  restarts: envs may start their next episode
        inside the launch (on_done="restart"); they no longer share one clock afterwards."""
        n_steps = self._n_steps(n_steps)
        self._set_trace(structs[0], trace, n_steps)
        self._b.cho = None
        self._b.flags = self._flags0
        clock, self._clock = self._clock, None        # the shadow clock survives only a call that went through
        ep0 = self.episode.clone() if (restarts and self._hist is not None) else None
        with torch.cuda.device(self.device):
            _lib.check(fn(self._ctx, C.byref(self._b), *[C.byref(s) if s is not None else None for s in structs], n_steps, self.minutes_per_step,
                          self.n_sub, self._stream()))
        if clock is not None and not restarts:
            self._clock = clock + n_steps * self.minutes_per_step
        self._hist_after_rollout()
        if ep0 is not None:                           # CGM_hist of an env whose last step ended its episode = [sample #0]
            self._hist_restart((self.episode != ep0) & (self.t == 0))

    def bb_constants(self):
        """Per-env BBController constants (basal_bolus_ctrller.py:54-64): basal = u2ss*BW/6000 U/min, CR and CF from
        Quest.csv; patients Quest.csv does not list get the reference's 'Average' row (CR 1/15, CF 1/50,
        u2ss 1.43, BW 57).  -> dict of tensors [n]."""
        basal, cr, cf = self._bb_rows()
        mk = lambda v: torch.as_tensor(v[self.patient_idx], dtype=self.dtype, device=self.device).contiguous()
        return {"basal": mk(basal), "cr": mk(cr), "cf": mk(cf)}

    def _bb_rows(self):
        """bb_constants() per row of self.names, in float64 before its cast -> numpy (basal, cr, cf)"""
        quest = params.quest_table()
        basal = np.empty(len(self.names)); cr = np.empty(len(self.names)); cf = np.empty(len(self.names))
        for k, name in enumerate(self.names):
            if name in quest:
                cr[k], cf[k] = quest[name][0], quest[name][1]
                basal[k] = params.basal_rate(self.table[k])
            else:
                cr[k], cf[k], basal[k] = 1.0 / 15.0, 1.0 / 50.0, 1.43 * 57.0 / 6000.0
        return basal, cr, cf

    def rollout_bb(self, n_steps, target=140.0, bb_state=None, stats=None, trace=None):
        """n_steps closed-loop BBController steps in one launch (SimObj.simulate with BBController: policy from
        the previous observation and the previous step's announced meal, then env.step).  bb_state: dict with
        basal, cr, cf (see bb_constants) and prev_meal [n] (created if None; prev_meal = 0 right after reset).
        Meals come from the meal tables (set_meals).  stats as in rollout_pid."""
        self._no_dopri5_rollout()
        bb_state, p = self._bb_struct(target, bb_state, stats)
        self._rollout(self._L.t1d_rollout_bb, (p,), n_steps, trace)
        return bb_state

    def new_policy_state(self, policy):
        """The state rollout_mlp carries for an MLPController, as it is right after reset(): every row of the CGM window
        holds the current observation, the insulin window and prev_meal are zero.  -> dict(cgm_hist [H, n], ins_hist [H, n],
        prev_meal [n])"""
        H = int(policy.history)
        return {"cgm_hist": self.cgm.unsqueeze(0).repeat(H, 1).contiguous(),
                "ins_hist": torch.zeros(H, self.n, dtype=self.dtype, device=self.device),
                "prev_meal": torch.zeros(self.n, dtype=self.dtype, device=self.device)}

    def _mlp_struct(self, who, policy, policy_state, stats=None):
        """the t1d_mlp of a policy and its state on this env, checked -> (struct, params tensor)"""
        npol = int(policy.n_policies)
        if self.n % npol or (self.n // npol) % 64:
            raise ValueError("%s: %d envs do not split into %d policies of a multiple of 64 envs each" % (who, self.n, npol))
        self._check_policy_state(policy_state, policy.history)
        params = policy.device_params(self.device, self.dtype)          # uploaded once per policy, device and dtype
        p = _lib.Mlp()
        policy.fill_struct(p)
        p.n_policies, p.envs_per_policy, p.n_params = npol, self.n // npol, params.shape[1]
        p.params = params.data_ptr()
        for k in ("cgm_hist", "ins_hist", "prev_meal"):
            setattr(p, k, policy_state[k].data_ptr())
        p.start_minute = self.start_minute.data_ptr() if self.start_minute is not None else None
        self._set_stats(p, stats)
        return p, params

    def _check_policy_state(self, policy_state, history):
        H = int(history)
        for k, shape in (("cgm_hist", (H, self.n)), ("ins_hist", (H, self.n)), ("prev_meal", (self.n,))):
            t = policy_state.get(k)
            if t is None or tuple(t.shape) != shape or t.dtype != self.dtype or t.device != self.device or not t.is_contiguous():
                raise ValueError("policy_state['%s'] must be a contiguous %s tensor of the env's dtype on its device" % (k, shape))

    def _feature_struct(self, features, policy_state):
        """the t1d_mlp of collect_pid / collect_bb, where no network runs: history, the feature scales and the windows (and
        the action_trace that the collector's builder sets); nothing else is read"""
        self._check_policy_state(policy_state, features.history)
        f = _lib.Mlp()
        f.history = int(features.history)
        f.cgm_mean, f.cgm_scale, f.ins_scale, f.cho_scale = features.cgm_mean, features.cgm_scale, features.ins_scale, features.cho_scale
        for k in ("cgm_hist", "ins_hist", "prev_meal"):
            setattr(f, k, policy_state[k].data_ptr())
        f.start_minute = self.start_minute.data_ptr() if self.start_minute is not None else None
        return f

    def _meal_bolus_struct(self, who, policy, trace=None, n_steps=0):
        """The t1d_meal_bolus of a policy with meal_bolus on this env, None for a policy without: the target of its
        BBController, cr and cf from bb_constants() (made once per env object and kept), and the "bolus" column of `trace`
        from the row the call starts at.  Call before _set_trace advances trace["row"]."""
        bb = getattr(policy, "meal_bolus", None)
        t = trace.get("bolus") if trace else None
        if bb is None:
            if t is not None:
                raise ValueError("%s: trace['bolus'] needs a policy with meal_bolus" % who)
            return None
        if getattr(self, "_bolus_constants", None) is None:
            k = self.bb_constants()
            self._bolus_constants = (k["cr"], k["cf"])
        m = _lib.MealBolus()
        m.target = float(bb.target)
        m.cr, m.cf = self._bolus_constants[0].data_ptr(), self._bolus_constants[1].data_ptr()
        m.bolus_trace = None
        if t is not None:
            row = int(trace.get("row", 0))
            if t.dtype != self.dtype or tuple(t.shape[1:]) != (self.n,) or t.shape[0] < row + n_steps or not t.is_contiguous():
                raise ValueError("trace['bolus'] must be contiguous [rows >= row + n_steps, %d] of %s" % (self.n, self.dtype))
            m.bolus_trace = t.data_ptr()
        return m

    def _env_output_struct(self, policy):
        """The t1d_env_output of a policy with relative_to="basal" on this env, None for a policy without: scale[i] =
        out_scale basal[i] and bias[i] = out_bias basal[i], basal the float64 word bb_constants() computes, the product formed
        in float64 and rounded once to the env's dtype.  Made once per (env, out_scale, out_bias) and kept."""
        if getattr(policy, "relative_to", None) is None:
            return None
        key = (float(policy.out_scale), float(policy.out_bias))
        kept = getattr(self, "_rel_constants", None)
        if kept is None or kept[0] != key:
            basal64 = self._bb_rows()[0][self.patient_idx]
            mk = lambda v: torch.as_tensor(v, dtype=self.dtype, device=self.device).contiguous()
            kept = self._rel_constants = (key, mk(key[0] * basal64), mk(key[1] * basal64))
        o = _lib.EnvOutput()
        o.scale, o.bias = kept[1].data_ptr(), kept[2].data_ptr()
        return o

    def policy_bolus(self, policy, policy_state):
        """The meal bolus [n], before the pump, that the next step of rollout_mlp / collect_mlp / rollout_mlp_dopri5 would
        ask for under a policy with meal_bolus (t1d_mlp_bolus, include/t1d.h): BBController's rule on the current observation
        (env.cgm) and policy_state["prev_meal"], by the roll-outs' own device function, so the word is theirs.  Nothing is
        changed and no step is taken; works in every mode.  A policy without meal_bolus asks for none: zeros.  The step()
        loop of a hybrid policy:

            st = env.new_policy_state(pol)
            env.step(env.policy_action(pol, st), env.policy_bolus(pol, st))
            pol.shift(st["cgm_hist"], st["ins_hist"], env.cgm, env.insulin); st["prev_meal"] = env.meal.clone()
        """
        m = self._meal_bolus_struct("policy_bolus", policy)
        if m is None:
            return torch.zeros(self.n, dtype=self.dtype, device=self.device)
        p, params = self._mlp_struct("policy_bolus", policy, policy_state)
        self._set_trace(p, None, 0)
        out = torch.empty(self.n, dtype=self.dtype, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._L.t1d_mlp_bolus(self._ctx, C.byref(self._b), C.byref(p), C.byref(m), C.c_void_p(out.data_ptr()), self._stream()))
        self._keep = (params, policy_state, out)
        return out

    def policy_action(self, policy, policy_state):
        """The basal [n], before the pump, that the next step of rollout_mlp / rollout_mlp_dopri5 would ask for
        (t1d_mlp_action, include/t1d.h): the network on the current observation (env.cgm), rows 1 .. of
        policy_state["cgm_hist"], its ins_hist and prev_meal, the env's clock and start_minute -- the roll-outs' own device
        code, so the word is theirs.  Nothing is changed and no step is taken; works in every mode.  A step() loop under
        the roll-outs' policy:

            st = env.new_policy_state(pol)
            u = env.policy_action(pol, st); env.step(u, 0 * u)
            pol.shift(st["cgm_hist"], st["ins_hist"], env.cgm, env.insulin); st["prev_meal"] = env.meal.clone()
        """
        o = self._env_output_struct(policy)
        if o is not None:                   # relative_to="basal": the word of the *_rel roll-outs
            return self._policy_alone("policy_action", self._L.t1d_mlp_action_rel, policy, policy_state, (self.n,), front=(C.byref(o),))
        return self._policy_alone("policy_action", self._L.t1d_mlp_action, policy, policy_state, (self.n,))

    def _policy_alone(self, who, fn, policy, policy_state, shape, front=()):
        """policy_action / policy_features: fn (t1d_mlp_action, t1d_mlp_action_rel, t1d_mlp_features) on the state as it is ->
        its output.  front: the arguments between the policy's struct and the output."""
        p, params = self._mlp_struct(who, policy, policy_state)
        self._set_trace(p, None, 0)
        out = torch.empty(*shape, dtype=self.dtype, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(fn(self._ctx, C.byref(self._b), C.byref(p), *front, C.c_void_p(out.data_ptr()), self._stream()))
        self._keep = (params, policy_state, out)
        return out

    def policy_features(self, policy, policy_state):
        """The features [F, n], F = 2 H + 3, that the next step of collect_mlp / collect_mlp_dopri5 would record in its
        "features" row (t1d_mlp_features, include/t1d.h), bit for bit: the device's own feature code -- its sinpi / cospi
        for the time-of-day pair -- on the current observation (env.cgm), rows 1 .. of policy_state["cgm_hist"], its
        ins_hist and prev_meal, the env's clock and start_minute.  Nothing is changed and no step is taken; works in every
        mode.  After a collect call these are the features of the state after its last step, which no trace row holds:
        what a critic needs for its bootstrap value at the cut (controller.gae):

            v_last = mlp_pre_output(vparams, env.policy_features(vpol, st)[None], vpol)[0]
        """
        return self._policy_alone("policy_features", self._L.t1d_mlp_features, policy, policy_state,
                                  (2 * int(policy.history) + 3, self.n))

    def rollout_mlp_dopri5(self, n_steps, policy, policy_state=None, stats=None, trace=None, max_minutes_per_launch=240):
        """rollout_mlp in the exact mode (t1d_rollout_mlp_dopri5): n_steps closed-loop steps under the in-kernel network with
        scipy's dopri5, every env at its own pace inside a launch -- SimObj.simulate as the reference would run it with that
        policy.  Results as a loop of policy_action(), step(u, 0) and the shift of the policy state, bit for bit.  Arguments
        and return value as rollout_mlp; h_carry, nfev and max_minutes_per_launch as in rollout_pid_dopri5.  A policy with
        meal_bolus runs t1d_rollout_mlp_dopri5_bolus: the loop with step(u, policy_bolus()); trace may hold "bolus".  Measured on an
        MI355X (160 steps, 1 Mi envs, H = 4, width 16; profiles/policy): 502 ms against 1 260 ms for that loop and 246 ms for
        rollout_pid_dopri5 -- lanes open their steps at different moments, and each moment runs the network for the few
        lanes that are there."""
        self._need_dopri5("rollout_mlp_dopri5")
        n_steps = self._n_steps(n_steps)
        if policy_state is None:
            policy_state = self.new_policy_state(policy)
        p, params = self._mlp_struct("rollout_mlp_dopri5", policy, policy_state, stats)
        m = self._meal_bolus_struct("rollout_mlp_dopri5", policy, trace, n_steps)
        o = self._env_output_struct(policy)
        if o is not None:
            self._rollout_dopri5(self._L.t1d_rollout_mlp_dopri5_rel, p, n_steps, trace, max_minutes_per_launch,
                                 extra=(C.byref(o), C.byref(m) if m is not None else None))
        elif m is None:
            self._rollout_dopri5(self._L.t1d_rollout_mlp_dopri5, p, n_steps, trace, max_minutes_per_launch)
        else:
            self._rollout_dopri5(self._L.t1d_rollout_mlp_dopri5_bolus, p, n_steps, trace, max_minutes_per_launch, extra=(C.byref(m),))
        self._keep = (params, policy_state)
        return policy_state

    def rollout_mlp(self, n_steps, policy, policy_state=None, stats=None, trace=None):
        """n_steps closed-loop steps in one launch under a feed-forward policy evaluated inside the kernel (t1d_rollout_mlp,
        include/t1d.h): policy is a controller.MLPController with one weight set, or with P of them -- env i then uses
        set i // (n // P), and n // P must be a multiple of 64.  policy_state: dict(cgm_hist, ins_hist, prev_meal) as
        new_policy_state() makes it (created if None: call right after reset()), updated in place and returned, so a
        roll-out can be cut anywhere and resumed.  The time-of-day features use the env's start_minute (0 if it has none).
        stats as in rollout_pid; trace may also hold "action" (new_trace).
        A policy built with meal_bolus= is a hybrid closed loop (t1d_rollout_mlp_bolus): beside the network's basal every
        announced meal gets BBController's bolus, formed in the kernel from the env's CR and CF (bb_constants()); trace may
        then hold "bolus", and the result is the loop of policy_action(), policy_bolus() and step(u, bolus), bit for bit.
        Measured on an MI355X (fp64 Dexcom, 160 steps, H = 4, width 16; profiles/policy): the bolus adds 2 - 3 % to the launch;
        against that loop one launch is 1.7 times faster at 64 Ki envs and LOSES at 1 Mi envs (701 against 409 us per step), as
        the bolus-free rollout_mlp does.
        A policy built with relative_to="basal" commands a multiple of each env's own basal rate (t1d_rollout_mlp_rel, with or
        without meal_bolus): basal = fma(scale[i], g(y), bias[i]) with scale = out_scale basal_i and bias = out_bias basal_i
        rounded once to the env's dtype, basal_i the word of bb_constants().  One weight set then serves a mixed cohort: the zero
        network with last bias 1 and meal_bolus=140 is rollout_bb for every patient at once, bit for bit.  collect_mlp,
        rollout_mlp_dopri5 and policy_action follow the policy in the same way; collect_mlp_dopri5 refuses it."""
        self._no_dopri5_rollout()
        n_steps = self._n_steps(n_steps)
        if policy_state is None:
            policy_state = self.new_policy_state(policy)
        p, params = self._mlp_struct("rollout_mlp", policy, policy_state, stats)
        m = self._meal_bolus_struct("rollout_mlp", policy, trace, n_steps)
        o = self._env_output_struct(policy)
        if o is not None:
            self._rollout(self._L.t1d_rollout_mlp_rel, (p, o, m), n_steps, trace)
        elif m is None:
            self._rollout(self._L.t1d_rollout_mlp, (p,), n_steps, trace)
        else:
            self._rollout(self._L.t1d_rollout_mlp_bolus, (p, m), n_steps, trace)
        self._keep = (params, policy_state)
        return policy_state

    def collect_mlp(self, n_steps, policy, sigma=None, explore_seed=None, policy_state=None, stats=None, trace=None,
                    on_done="continue", days=2, terminal_obs=None, episode_stats=None, reset_outputs=False):
        """A batch of trajectories for a policy-gradient trainer in one launch (t1d_collect_mlp, include/t1d.h): rollout_mlp
        with exploration noise, the reward and done of every step, the features the network saw, and episodes that end.
        sigma: None (no noise, no draw), a float or a tensor [P]: the action is out_scale g(y + sigma eps) + out_bias with
        eps ~ N(0, 1) drawn per env and step from explore_seed (default seed ^ 0x5851F42D4C957F2D), the env's global id, its
        episode counter and its clock -- not from the cut, the shard or the neighbours.  MLPController.log_prob(eps, sigma)
        is the log-density of the pre-output sample.
        on_done: "continue" = episodes never end, as rollout_mlp; "restart" = an env whose step comes back done starts its
        next episode before its next step as restart_done(days, terminal_obs, episode_stats, reset_outputs) would, and its
        policy state becomes that of new_policy_state() after a reset.  The result is that of a loop of rollout_mlp(1),
        restart_done() and the torch reset of policy_state, bit for bit.  The finished env is restarted by its own lane, in a
        wave that waits for it.  Measured on an MI355X (fp64 Dexcom, 32 steps, profiles/collect): at 64 Ki envs one launch is
        1.75 - 1.8 times faster than that loop; at 1 Mi envs it LOSES to the loop where more than about 0.85 % of the envs
        finish per step (episodes shorter than ~120 steps: by 22 % on the hypo workload, 1.6 % per step) and wins below.
        trace: as rollout_mlp, and "reward", "done", "eps", "features" (new_trace).  Row s always describes step s: for an env
        that finished there trace["cgm"][s] is the terminal observation, the new episode's first one shows in
        trace["features"][s + 1] and in env.cgm.  A policy with meal_bolus runs t1d_collect_mlp_bolus (see rollout_mlp; "bolus"
        in trace); a restarted env has prev_meal = 0, hence no bolus on its first step.  -> policy_state.

        The PPO ratio from a collected batch, with the network evaluated again on the device by the collector's own code
        (controller.mlp_pre_output: differentiable in the weights, no activations stored; at unchanged weights y_new is
        y_old bit for bit and the ratio exactly 1):

            from simglucose_amd.controller import mlp_pre_output
            tr = env.new_trace(K, columns=("reward", "done", "eps", "features"), history=pol.history)
            env.collect_mlp(K, pol, sigma=sig, trace=tr, on_done="restart")
            f, eps = tr["features"][1:], tr["eps"][1:]                    # [K, F, n], [K, n]
            old_params = pol.device_params(env.device, env.dtype)          # [P, n_params], what the collector ran
            new_params = old_params.clone().requires_grad_(True)           # the weights being trained
            y_old = mlp_pre_output(old_params, f, pol)                     # [K, n], no grad
            z = y_old + sig * eps                                          # the pre-output sample that was acted on
            old = MLPController.log_prob((z - y_old) / sig, sig)           # log pi_old(a | s), formed as `new` is
            y_new = mlp_pre_output(new_params, f, pol)
            new = MLPController.log_prob((z - y_new) / sig_new, sig_new)
            ratio = (new - old).exp()
        """
        self._no_dopri5_rollout()
        policy_state, p, g, keep = self._collect_structs("collect_mlp", n_steps, policy, policy_state, stats, trace, on_done, days,
                                                         terminal_obs, episode_stats, reset_outputs, draw=(sigma, explore_seed))
        m = self._meal_bolus_struct("collect_mlp", policy, trace, self._n_steps(n_steps))
        o = self._env_output_struct(policy)
        if o is not None:
            self._rollout(self._L.t1d_collect_mlp_rel, (p, g, o, m), n_steps, trace, restarts=on_done == "restart")
        elif m is None:
            self._rollout(self._L.t1d_collect_mlp, (p, g), n_steps, trace, restarts=on_done == "restart")
        else:
            self._rollout(self._L.t1d_collect_mlp_bolus, (p, g, m), n_steps, trace, restarts=on_done == "restart")
        self._keep = keep
        return policy_state

    def collect_mlp_limit(self, n_steps, policy, max_episode_steps, cut_features=None, sigma=None, explore_seed=None,
                          policy_state=None, stats=None, trace=None, on_done="restart", days=2, terminal_obs=None,
                          episode_stats=None, reset_outputs=False):
        """collect_mlp(on_done="restart") with a time limit on every episode (t1d_collect_mlp_limit, include/t1d.h; one entry
        point and one kernel family for the plain, the hybrid and the relative policy).  max_episode_steps = L >= 1: an env
        that did not finish and whose clock has reached L * minutes_per_step when a step closes is cut (truncated).  Its row
        has done = 0 and trace["truncated"] = 1 (termination wins, never both); cut_features (a contiguous [F, n] tensor of
        the env's dtype, or None) receives, for the cut envs only, the features of the state the episode ended in -- what
        policy_features() would return at that moment, bit for bit: what the critic bootstraps from (controller.gae:
        truncated=, cut_value=).  The cut env then goes through what a finished one goes through.  on_done must be "restart"
        (a cut env starts its next episode) and n_steps <= L (an env is then cut at most once per call, so one cut_features
        column per env is enough; a longer batch takes several calls): else ValueError before anything is launched.  Every
        other argument, and the return value, as collect_mlp; trace may hold "truncated" (new_trace).  The result is that of
        n_steps times this loop, bit for bit, wherever the call is cut into launches:

            env.rollout_mlp(1, pol, policy_state=st)         # or collect_mlp(1, ..., on_done="continue") with sigma
            cut = ~env.done.bool() & (env.t >= L * env.minutes_per_step)
            cut_features[:, cut] = env.policy_features(pol, st)[:, cut]
            env.restart_done(mask=env.done.bool() | cut, ...)
            ...                                              # new_policy_state() for the masked envs

        With a limit no env reaches, the result is collect_mlp(on_done="restart")'s, bit for bit.  A method of its own and not
        two keywords of collect_mlp, whose parameter list is that of collect_mlp_dopri5 and stays so.  The other collectors have
        the same limit under the same rules: collect_pid_limit, collect_bb_limit, collect_mlp_dopri5_limit,
        collect_pid_dopri5_limit and collect_bb_dopri5_limit; what has none is the exact MLP collector under a meal_bolus or
        relative_to policy, which collect_mlp_dopri5_limit refuses as collect_mlp_dopri5 does.  Measurements:
        profiles/collect/README.md."""
        self._no_dopri5_rollout()
        lim = self._time_limit_struct(n_steps, policy, trace, on_done, max_episode_steps, cut_features)
        policy_state, p, g, keep = self._collect_structs("collect_mlp_limit", n_steps, policy, policy_state, stats, trace, on_done, days,
                                                         terminal_obs, episode_stats, reset_outputs, draw=(sigma, explore_seed))
        m = self._meal_bolus_struct("collect_mlp_limit", policy, trace, self._n_steps(n_steps))
        o = self._env_output_struct(policy)
        self._rollout(self._L.t1d_collect_mlp_limit, (p, g, o, m, lim), n_steps, trace, restarts=True)
        self._keep = keep + (cut_features,)
        return policy_state

    def _time_limit_struct(self, n_steps, policy, trace, on_done, max_episode_steps, cut_features, who="collect_mlp_limit"):
        """The t1d_time_limit of the six *_limit collectors, checked before anything is launched; `who` is the caller's name in
        the messages, `policy` the network that acts or the controller's features=.  Call before _set_trace advances
        trace["row"]: "truncated" is written from the row the call starts at."""
        t = trace.get("truncated") if trace else None
        n_steps, L = self._n_steps(n_steps), int(max_episode_steps)
        if L < 1:
            raise ValueError("%s: max_episode_steps must be at least 1" % who)
        if on_done != "restart":
            raise ValueError("%s: max_episode_steps needs on_done='restart' (a cut env starts its next episode)" % who)
        if n_steps > L:
            raise ValueError("%s: n_steps must not exceed max_episode_steps (an env is cut at most once per call); "
                             "take the batch in several calls" % who)
        lim = _lib.TimeLimit()
        lim.max_minutes, lim.reserved = L * self.minutes_per_step, 0
        lim.cut_trace = lim.cut_feat = None
        if cut_features is not None:
            if policy is None:
                raise ValueError("%s: features= takes the MLPController whose history and scales form the features" % who)
            F = 2 * int(policy.history) + 3
            if not isinstance(cut_features, torch.Tensor) or cut_features.dtype != self.dtype or cut_features.device != self.device \
                    or tuple(cut_features.shape) != (F, self.n) or not cut_features.is_contiguous():
                raise ValueError("%s: cut_features must be a contiguous [%d, %d] tensor of %s on the env's device" % (who, F, self.n, self.dtype))
            lim.cut_feat = cut_features.data_ptr()
        if t is not None:
            row = int(trace.get("row", 0))
            if t.dtype != torch.uint8 or tuple(t.shape[1:]) != (self.n,) or t.shape[0] < row + n_steps or not t.is_contiguous():
                raise ValueError("trace['truncated'] must be contiguous [rows >= row + n_steps, %d] of torch.uint8" % self.n)
            lim.cut_trace = t.data_ptr()
        return lim

    def _collect_structs(self, who, n_steps, policy, policy_state, stats, trace, on_done, days, terminal_obs, episode_stats,
                         reset_outputs, draw, keep_h_carry=False):
        """The t1d_mlp and t1d_collect of the six collectors, checked.  draw = (sigma, explore_seed): `policy` is the network
        that acts, the call may record "eps", and the t1d_mlp's own five trace columns are left to _set_trace.  draw = None
        (collect_pid / collect_bb and their *_dopri5 forms): a controller acts, `policy` only forms the features, `stats` belong to the controller's
        struct, there is no "eps" column and "action" is set here.  keep_h_carry: the exact mode, where a restart zeroes it.
        -> (policy_state, t1d_mlp, t1d_collect, what must stay alive until the launch has run)"""
        n_steps = self._n_steps(n_steps)
        if on_done not in ("continue", "restart"):
            raise ValueError("on_done must be 'continue' or 'restart'")
        if draw is None:
            if policy is None:
                raise ValueError("%s: features= takes the MLPController whose history and scales form the features" % who)
            if trace and trace.get("eps") is not None:
                raise ValueError("%s: a controller draws no exploration noise, there is no 'eps' column" % who)
        if policy_state is None:
            policy_state = self.new_policy_state(policy)
        g = _lib.Collect()
        params = sigma = None
        if draw is None:
            p = self._feature_struct(policy, policy_state)
        else:
            p, params = self._mlp_struct(who, policy, policy_state, stats)
            sigma, explore_seed = draw
            g.explore_seed = (self.seed ^ 0x5851F42D4C957F2D if explore_seed is None else int(explore_seed)) & 0xFFFFFFFFFFFFFFFF
            if sigma is not None:
                sigma = torch.as_tensor(sigma, dtype=self.dtype).detach().to(self.device).expand(int(policy.n_policies)).contiguous()
                g.sigma = sigma.data_ptr()
        g.on_done, g.reserved = (_lib.T1D_COLLECT_RESTART if on_done == "restart" else _lib.T1D_COLLECT_CONTINUE), 0
        r = None
        if on_done == "restart":
            if self.noise == "host" or self.normals is not None:
                raise _lib.T1DError("%s(on_done='restart') draws every episode on the device: not available with host normals" % who)
            r = self._restart_struct(int(days), terminal_obs, episode_stats or {}, reset_outputs, who)
            if not keep_h_carry:
                r.h_carry = None
            g.restart = C.pointer(r)
            p.start_minute = r.start_minute          # _restart_struct creates the array for an env that had none
            self._b.x0_override = None
        row = int(trace.get("row", 0)) if trace else 0
        F = 2 * int(policy.history) + 3
        for k, tgt, fld, dt, shape in (("reward", g, "reward_trace", self.dtype, (self.n,)), ("done", g, "done_trace", torch.uint8, (self.n,)),
                                       ("eps", g, "eps_trace", self.dtype, (self.n,)), ("features", g, "feat_trace", self.dtype, (F, self.n)),
                                       ("action", p, "action_trace", self.dtype, (self.n,))):
            t = trace.get(k) if trace and (k != "action" or draw is None) else None
            if t is not None:
                if t.dtype != dt or tuple(t.shape[1:]) != shape or t.shape[0] < row + n_steps or not t.is_contiguous():
                    raise ValueError("trace['%s'] must be contiguous [rows >= row + n_steps, %s] of %s" % (k, ", ".join(map(str, shape)), dt))
                setattr(tgt, fld, t.data_ptr())
        return policy_state, p, g, (params, policy_state, sigma, r, terminal_obs, episode_stats, stats, trace)

    def _collect_ctrl(self, who, fn, ctl, ctl_state, n_steps, features, policy_state, stats, trace, on_done, days, terminal_obs,
                      episode_stats, reset_outputs, lim=None, cut_features=None):
        """collect_pid / collect_bb: fn (t1d_collect_pid, t1d_collect_bb) with the controller's struct ctl -> policy_state.
        lim: the t1d_time_limit of the *_limit forms (_time_limit_struct, made before anything else of the call), whose fn
        takes it behind the t1d_collect; cut_features is kept alive with the rest"""
        policy_state, f, g, keep = self._collect_structs(who, n_steps, features, policy_state, stats, trace, on_done, days,
                                                         terminal_obs, episode_stats, reset_outputs, draw=None)
        self._rollout(fn, (ctl, f, g) if lim is None else (ctl, f, g, lim), n_steps, trace, restarts=on_done == "restart")
        self._keep = keep + (ctl_state, cut_features)
        return policy_state

    def collect_pid(self, n_steps, P, I, D, target=140.0, features=None, pid_state=None, policy_state=None, stats=None, trace=None,
                    on_done="continue", days=2, terminal_obs=None, episode_stats=None, reset_outputs=False):
        """rollout_pid with what collect_mlp adds, in one launch (t1d_collect_pid, include/t1d.h): the PID controller drives
        the envs while every step records the features a network would have been given and the insulin the controller
        asked for -- the data a policy is fitted to before it explores -- and the reward and done of every step, with
        episodes that end (on_done="restart") under collect_mlp's rules.
        features: an MLPController; only its history and feature scales are used (no network runs, and n need not be a
        multiple of 64).  policy_state: the feature windows, dict(cgm_hist, ins_hist, prev_meal) as new_policy_state(features)
        makes it (created if None: call right after reset()).  pid_state, stats as in rollout_pid; on_done, days,
        terminal_obs, episode_stats, reset_outputs as in collect_mlp.  A restarted env's integ and prev become 0.
        trace: new_trace's bg, cgm, cho, insulin, action, reward, done, features; "action" is basal + bolus of the step,
        before the pump -- with "features" of the same row the regression sample for a network with identity output.
        The result is that of a loop of policy_features(), rollout_pid(1) with rollout_launches = 0, the shift of the
        windows, restart_done() and the torch reset of both states, bit for bit.  Measured on an MI355X (collect_bb, fp64
        Dexcom, 32 steps, profiles/collect): at 64 Ki envs one launch is 2.2 - 3.3 times faster than that loop; at 1 Mi envs
        it wins by 20 % under the stock basal-bolus constants (0.27 % of the envs finish per step) and LOSES by 12 % where
        1 % finish per step, like collect_mlp.  -> (pid_state, policy_state)"""
        self._no_dopri5_rollout()
        self._no_per_env_gains("collect_pid", P, I, D, target)
        pid_state, p = self._pid_struct(P, I, D, target, pid_state, stats)
        policy_state = self._collect_ctrl("collect_pid", self._L.t1d_collect_pid, p, pid_state, n_steps, features, policy_state, stats,
                                          trace, on_done, days, terminal_obs, episode_stats, reset_outputs)
        return pid_state, policy_state

    def collect_bb(self, n_steps, target=140.0, features=None, bb_state=None, policy_state=None, stats=None, trace=None,
                   on_done="continue", days=2, terminal_obs=None, episode_stats=None, reset_outputs=False):
        """rollout_bb with what collect_mlp adds, in one launch (t1d_collect_bb, include/t1d.h): the basal-bolus controller
        drives the envs; everything else as collect_pid.  bb_state as in rollout_bb (created from bb_constants() if None);
        a restarted env's bb_state["prev_meal"] becomes 0.  The warm start of a policy:

            tr = env.new_trace(K, columns=("action", "features"), history=pol.history)
            env.collect_bb(K, features=pol, trace=tr, on_done="restart")
            loss = value_loss(params, tr["features"][1:], pol, target=tr["action"][1:])

        -> (bb_state, policy_state)"""
        self._no_dopri5_rollout()
        bb_state, p = self._bb_struct(target, bb_state, stats)
        policy_state = self._collect_ctrl("collect_bb", self._L.t1d_collect_bb, p, bb_state, n_steps, features, policy_state, stats,
                                          trace, on_done, days, terminal_obs, episode_stats, reset_outputs)
        return bb_state, policy_state

    def collect_pid_limit(self, n_steps, P, I, D, max_episode_steps, cut_features=None, target=140.0, features=None, pid_state=None,
                          policy_state=None, stats=None, trace=None, on_done="restart", days=2, terminal_obs=None,
                          episode_stats=None, reset_outputs=False):
        """collect_pid(on_done="restart") with collect_mlp_limit's time limit on every episode (t1d_collect_pid_limit,
        include/t1d.h): the classical baseline under the rules a policy trained with collect_mlp_limit(L) is scored by.
        max_episode_steps = L, cut_features (contiguous [F, n] of the env's dtype, F from features=, or None), the "truncated"
        trace column, on_done="restart" only and n_steps <= L: as collect_mlp_limit, ValueError before anything is launched.
        A cut env goes through what a finished one goes through: its integ and prev become 0.  The result is that of n_steps
        times this loop, bit for bit, wherever the call is cut into launches:

            f = env.policy_features(features, st); env.rollout_pid(1, P, I, D, pid_state=ps)   # rollout_launches = 0
            ...                                              # the shift of the windows in st, prev_meal = env.meal
            cut = ~env.done.bool() & (env.t >= L * env.minutes_per_step)
            cut_features[:, cut] = env.policy_features(features, st)[:, cut]
            env.restart_done(mask=env.done.bool() | cut, ...)
            ...                                              # new_policy_state() and a zeroed pid_state for the masked envs

        With a limit no env reaches, the result is collect_pid(on_done="restart")'s, bit for bit.  Every other argument, and
        the return value, as collect_pid.  Measurements: profiles/collect/README.md.  -> (pid_state, policy_state)"""
        self._no_dopri5_rollout()
        self._no_per_env_gains("collect_pid_limit", P, I, D, target)
        lim = self._time_limit_struct(n_steps, features, trace, on_done, max_episode_steps, cut_features, "collect_pid_limit")
        pid_state, p = self._pid_struct(P, I, D, target, pid_state, stats)
        policy_state = self._collect_ctrl("collect_pid_limit", self._L.t1d_collect_pid_limit, p, pid_state, n_steps, features,
                                          policy_state, stats, trace, on_done, days, terminal_obs, episode_stats, reset_outputs,
                                          lim, cut_features)
        return pid_state, policy_state

    def collect_bb_limit(self, n_steps, max_episode_steps, cut_features=None, target=140.0, features=None, bb_state=None,
                         policy_state=None, stats=None, trace=None, on_done="restart", days=2, terminal_obs=None, episode_stats=None,
                         reset_outputs=False):
        """collect_bb(on_done="restart") with the time limit (t1d_collect_bb_limit): everything as collect_pid_limit, the loop
        with rollout_bb(1); a cut env's bb_state["prev_meal"] becomes 0.  The baseline beside a policy trained under L, and a
        critic's warm start with states to bootstrap from:

            cut = torch.zeros(F, env.n, dtype=env.dtype, device=env.device)
            tr = env.new_trace(K, columns=("reward", "done", "truncated", "features"), history=pol.history)
            env.collect_bb_limit(K, L, cut_features=cut, features=pol, trace=tr, episode_stats=es)     # K <= L

        -> (bb_state, policy_state)"""
        self._no_dopri5_rollout()
        lim = self._time_limit_struct(n_steps, features, trace, on_done, max_episode_steps, cut_features, "collect_bb_limit")
        bb_state, p = self._bb_struct(target, bb_state, stats)
        policy_state = self._collect_ctrl("collect_bb_limit", self._L.t1d_collect_bb_limit, p, bb_state, n_steps, features,
                                          policy_state, stats, trace, on_done, days, terminal_obs, episode_stats, reset_outputs,
                                          lim, cut_features)
        return bb_state, policy_state

    def collect_mlp_dopri5(self, n_steps, policy, sigma=None, explore_seed=None, policy_state=None, stats=None, trace=None,
                           on_done="continue", days=2, terminal_obs=None, episode_stats=None, reset_outputs=False,
                           max_minutes_per_launch=240):
        """collect_mlp in the exact mode (t1d_collect_mlp_dopri5, include/t1d.h): trajectories for a policy-gradient trainer
        with scipy's dopri5, every env at its own pace inside a launch -- through its minutes, its steps and, with
        on_done="restart", its episodes.  Arguments, draws, trace columns and return value as collect_mlp; h_carry, nfev (summed
        over the whole call, across an env's episodes) and max_minutes_per_launch as in rollout_pid_dopri5 -- the cut changes no
        result.  A restarted env's h_carry becomes 0: its first minute probes the step size, as after reset().  The result is
        that of a loop of rollout_mlp_dopri5(1), restart_done() and the torch reset of policy_state, bit for bit (for envs
        whose solver does not give up); with sigma=None and on_done="continue" it is rollout_mlp_dopri5's.  Measurements:
        profiles/collect (exact_collect_bench.json).  A policy with meal_bolus is refused: the exact mode's collector has no
        meal bolus (there is no t1d_collect_mlp_dopri5_bolus), and it does not drop it silently."""
        return self._collect_mlp_dopri5("collect_mlp_dopri5", "t1d_collect_mlp_dopri5", n_steps, policy, sigma, explore_seed,
                                        policy_state, stats, trace, on_done, days, terminal_obs, episode_stats, reset_outputs,
                                        max_minutes_per_launch)

    def _collect_mlp_dopri5(self, who, fn, n_steps, policy, sigma, explore_seed, policy_state, stats, trace, on_done, days, terminal_obs,
                            episode_stats, reset_outputs, max_minutes_per_launch, limit=None):
        """collect_mlp_dopri5 and, with limit = (max_episode_steps, cut_features), collect_mlp_dopri5_limit, whose entry point fn
        (by name: an env of the other mode is turned away before anything of it is read) takes a t1d_time_limit behind the
        t1d_collect -- the same one in every launch the call is cut into -> policy_state"""
        self._need_dopri5(who)
        if getattr(policy, "meal_bolus", None) is not None:
            raise _lib.T1DError("%s: the exact-mode collector has no meal bolus (there is no t1d_collect_mlp_dopri5_bolus): "
                                "a policy with meal_bolus takes rollout_mlp_dopri5, or collect_mlp on a fixed-step env" % who)
        if getattr(policy, "relative_to", None) is not None:
            raise _lib.T1DError("%s: the exact-mode collector has no patient-relative output (relative_to=%r; there is no "
                                "t1d_collect_mlp_dopri5_rel): such a policy takes rollout_mlp_dopri5, or collect_mlp on a fixed-step env"
                                % (who, policy.relative_to))
        lim = None if limit is None else self._time_limit_struct(n_steps, policy, trace, on_done, limit[0], limit[1], who)
        policy_state, p, g, keep = self._collect_structs(who, n_steps, policy, policy_state, stats, trace, on_done,
                                                         days, terminal_obs, episode_stats, reset_outputs, draw=(sigma, explore_seed),
                                                         keep_h_carry=True)
        self._rollout_dopri5(getattr(self._L, fn), p, n_steps, trace, max_minutes_per_launch,
                             extra=(C.byref(g),) if lim is None else (C.byref(g), C.byref(lim)), restarts=on_done == "restart")
        self._keep = keep + (limit,)
        return policy_state

    def collect_mlp_dopri5_limit(self, n_steps, policy, max_episode_steps, cut_features=None, sigma=None, explore_seed=None,
                                 policy_state=None, stats=None, trace=None, on_done="restart", days=2, terminal_obs=None,
                                 episode_stats=None, reset_outputs=False, max_minutes_per_launch=240):
        """collect_mlp_dopri5(on_done="restart") with collect_mlp_limit's time limit on every episode
        (t1d_collect_mlp_dopri5_limit, include/t1d.h): a policy trained under a limit, scored or fine-tuned on the exact
        integrator under the same limit.  max_episode_steps = L, cut_features, the "truncated" trace column, on_done="restart"
        only and n_steps <= L: as collect_mlp_limit, ValueError before anything is launched.  A cut env goes through what a
        finished one goes through; its h_carry becomes 0.  The call is cut into launches as collect_mlp_dopri5 is, each under
        the same limit; an env is still cut at most once per call.  The result is that of n_steps times this loop, bit for bit
        (for envs whose solver does not give up):

            env.rollout_mlp_dopri5(1, pol, policy_state=st)  # or collect_mlp_dopri5(1, ..., on_done="continue") with sigma
            cut = ~env.done.bool() & (env.t >= L * env.minutes_per_step)
            cut_features[:, cut] = env.policy_features(pol, st)[:, cut]
            env.restart_done(mask=env.done.bool() | cut, ...)
            ...                                              # new_policy_state() for the masked envs

        With a limit no env reaches, the result is collect_mlp_dopri5(on_done="restart")'s, bit for bit.  A policy with
        meal_bolus or relative_to is refused as collect_mlp_dopri5 refuses it: that is what still has no time limit in the
        exact mode.  Measurements: profiles/collect/README.md."""
        return self._collect_mlp_dopri5("collect_mlp_dopri5_limit", "t1d_collect_mlp_dopri5_limit", n_steps, policy, sigma,
                                        explore_seed, policy_state, stats, trace, on_done, days, terminal_obs, episode_stats,
                                        reset_outputs, max_minutes_per_launch, limit=(max_episode_steps, cut_features))

    def _collect_ctrl_dopri5(self, who, fn, ctl, ctl_state, n_steps, features, policy_state, stats, trace, on_done, days,
                             terminal_obs, episode_stats, reset_outputs, max_minutes_per_launch, lim=None, cut_features=None):
        """collect_pid_dopri5 / collect_bb_dopri5: fn with the controller's struct ctl, whose trace_row -- the row of every
        trace of these calls -- _rollout_dopri5 advances from launch to launch; the feature struct holds pointers only and
        needs nothing advanced.  lim, cut_features: as in _collect_ctrl; every launch takes the same t1d_time_limit
        -> policy_state"""
        policy_state, f, g, keep = self._collect_structs(who, n_steps, features, policy_state, stats, trace, on_done, days,
                                                         terminal_obs, episode_stats, reset_outputs, draw=None, keep_h_carry=True)
        self._rollout_dopri5(fn, ctl, n_steps, trace, max_minutes_per_launch,
                             extra=(C.byref(f), C.byref(g)) if lim is None else (C.byref(f), C.byref(g), C.byref(lim)),
                             restarts=on_done == "restart")
        self._keep = keep + (ctl_state, cut_features)
        return policy_state

    def collect_pid_dopri5(self, n_steps, P, I, D, target=140.0, features=None, pid_state=None, policy_state=None, stats=None,
                           trace=None, on_done="continue", days=2, terminal_obs=None, episode_stats=None, reset_outputs=False,
                           max_minutes_per_launch=240):
        """collect_pid in the exact mode (t1d_collect_pid_dopri5, include/t1d.h): the PID controller drives the envs on scipy's
        dopri5, every env at its own pace inside a launch -- through its minutes, its steps and, with on_done="restart", its
        episodes -- while every step records the features a network would have been given, basal + bolus, reward and done.
        Arguments, trace columns and return value as collect_pid (n need not be a multiple of 64); h_carry, nfev (summed over
        the whole call, across an env's episodes) and max_minutes_per_launch as in rollout_pid_dopri5 -- the cut changes no
        result.  A restarted env's h_carry, integ and prev become 0.  The result is that of a loop of policy_features(),
        rollout_pid_dopri5(1), the shift of the windows, restart_done() and the torch reset of both states, bit for bit (for
        envs whose solver does not give up); with on_done="continue" the env, pid_state, stats and the four roll-out columns
        are rollout_pid_dopri5's.  Measurements: profiles/collect (exact_ctrl_collect_bench.json).
        -> (pid_state, policy_state)"""
        self._need_dopri5("collect_pid_dopri5")
        self._no_per_env_gains("collect_pid_dopri5", P, I, D, target)
        pid_state, p = self._pid_struct(P, I, D, target, pid_state, stats)
        policy_state = self._collect_ctrl_dopri5("collect_pid_dopri5", self._L.t1d_collect_pid_dopri5, p, pid_state, n_steps,
                                                 features, policy_state, stats, trace, on_done, days, terminal_obs, episode_stats,
                                                 reset_outputs, max_minutes_per_launch)
        return pid_state, policy_state

    def collect_bb_dopri5(self, n_steps, target=140.0, features=None, bb_state=None, policy_state=None, stats=None, trace=None,
                          on_done="continue", days=2, terminal_obs=None, episode_stats=None, reset_outputs=False,
                          max_minutes_per_launch=240):
        """collect_bb in the exact mode (t1d_collect_bb_dopri5, include/t1d.h): the basal-bolus controller on scipy's dopri5 --
        the reference's own regression run -- with what collect_bb records; everything else as collect_pid_dopri5.  A restarted
        env's bb_state["prev_meal"] becomes 0.  The warm start of a policy that is then trained and scored with
        collect_mlp_dopri5:

            tr = env.new_trace(K, columns=("action", "features"), history=pol.history)
            env.collect_bb_dopri5(K, features=pol, trace=tr, on_done="restart")
            loss = value_loss(params, tr["features"][1:], pol, target=tr["action"][1:])

        -> (bb_state, policy_state)"""
        self._need_dopri5("collect_bb_dopri5")
        bb_state, p = self._bb_struct(target, bb_state, stats)
        policy_state = self._collect_ctrl_dopri5("collect_bb_dopri5", self._L.t1d_collect_bb_dopri5, p, bb_state, n_steps,
                                                 features, policy_state, stats, trace, on_done, days, terminal_obs, episode_stats,
                                                 reset_outputs, max_minutes_per_launch)
        return bb_state, policy_state

    def collect_pid_dopri5_limit(self, n_steps, P, I, D, max_episode_steps, cut_features=None, target=140.0, features=None,
                                 pid_state=None, policy_state=None, stats=None, trace=None, on_done="restart", days=2,
                                 terminal_obs=None, episode_stats=None, reset_outputs=False, max_minutes_per_launch=240):
        """collect_pid_dopri5(on_done="restart") with the time limit of collect_pid_limit (t1d_collect_pid_dopri5_limit,
        include/t1d.h): max_episode_steps, cut_features, "truncated" and the refusals as there; a cut env's h_carry, integ and
        prev become 0.  The call is cut into launches as collect_pid_dopri5 is, each under the same limit.  The result is that
        of collect_pid_limit's loop with rollout_pid_dopri5(1), bit for bit (for envs whose solver does not give up); with a
        limit no env reaches it is collect_pid_dopri5(on_done="restart")'s.  -> (pid_state, policy_state)"""
        self._need_dopri5("collect_pid_dopri5_limit")
        self._no_per_env_gains("collect_pid_dopri5_limit", P, I, D, target)
        lim = self._time_limit_struct(n_steps, features, trace, on_done, max_episode_steps, cut_features, "collect_pid_dopri5_limit")
        pid_state, p = self._pid_struct(P, I, D, target, pid_state, stats)
        policy_state = self._collect_ctrl_dopri5("collect_pid_dopri5_limit", self._L.t1d_collect_pid_dopri5_limit, p, pid_state,
                                                 n_steps, features, policy_state, stats, trace, on_done, days, terminal_obs,
                                                 episode_stats, reset_outputs, max_minutes_per_launch, lim, cut_features)
        return pid_state, policy_state

    def collect_bb_dopri5_limit(self, n_steps, max_episode_steps, cut_features=None, target=140.0, features=None, bb_state=None,
                                policy_state=None, stats=None, trace=None, on_done="restart", days=2, terminal_obs=None,
                                episode_stats=None, reset_outputs=False, max_minutes_per_launch=240):
        """collect_bb_dopri5(on_done="restart") with the time limit of collect_bb_limit (t1d_collect_bb_dopri5_limit):
        everything as collect_pid_dopri5_limit; a cut env's bb_state["prev_meal"] becomes 0.  -> (bb_state, policy_state)"""
        self._need_dopri5("collect_bb_dopri5_limit")
        lim = self._time_limit_struct(n_steps, features, trace, on_done, max_episode_steps, cut_features, "collect_bb_dopri5_limit")
        bb_state, p = self._bb_struct(target, bb_state, stats)
        policy_state = self._collect_ctrl_dopri5("collect_bb_dopri5_limit", self._L.t1d_collect_bb_dopri5_limit, p, bb_state,
                                                 n_steps, features, policy_state, stats, trace, on_done, days, terminal_obs,
                                                 episode_stats, reset_outputs, max_minutes_per_launch, lim, cut_features)
        return bb_state, policy_state

    def _rollout_dopri5(self, fn, p, n_steps, trace, max_minutes_per_launch, extra=(), restarts=False):
        """the launches of one exact-mode roll-out: whole steps, at most max_minutes_per_launch simulated minutes each.
        State, controller state and h_carry carry over, so the cut changes no result; nfev is summed over the launches.
        extra: the arguments between the controller's struct and h_carry (the collector's t1d_collect).  restarts: as in
        _rollout."""
        n_steps = self._n_steps(n_steps)
        per = max(1, int(max_minutes_per_launch) // self.minutes_per_step)
        self._set_trace(p, trace, n_steps)
        self._b.cho = None
        self._b.flags = self._flags0
        clock, self._clock = self._clock, None
        ep0 = self.episode.clone() if (restarts and self._hist is not None) else None
        total = None if n_steps <= per else torch.zeros_like(self.nfev)
        with torch.cuda.device(self.device):
            done = 0
            while done < n_steps:
                k = min(per, n_steps - done)
                _lib.check(fn(self._ctx, C.byref(self._b), C.byref(p), *extra, C.c_void_p(self.h_carry.data_ptr()),
                              C.c_void_p(self.nfev.data_ptr()), k, self.minutes_per_step, self._stream()))
                if total is not None:
                    total += self.nfev
                p.trace_row += k
                done += k
        if total is not None:
            self.nfev.copy_(total)
        if clock is not None and not restarts:         # restarted envs no longer share the clock
            self._clock = clock + n_steps * self.minutes_per_step
        self._hist_after_rollout()
        if ep0 is not None:                            # CGM_hist of an env whose last step ended its episode = [sample #0]
            self._hist_restart((self.episode != ep0) & (self.t == 0))

    def _need_dopri5(self, who):
        if self.integrator != "dopri5":
            raise _lib.T1DError("%s needs an env built with integrator='dopri5' (the fixed-step envs take %s)"
                                % (who, who.replace("_dopri5", "")))

    def rollout_pid_dopri5(self, n_steps, P, I=None, D=None, target=140.0, pid_state=None, stats=None, trace=None,
                           max_minutes_per_launch=240):
        """rollout_pid in the exact mode (t1d_rollout_pid_dopri5): n_steps closed-loop PID steps with scipy's dopri5, every
        env at its own pace inside a launch; results as a step() loop with the controller evaluated operation by operation
        in between, bit for bit.  Arguments and return value as rollout_pid; uses the env's h_carry and leaves the RHS
        evaluations of the whole call in nfev.  max_minutes_per_launch: the call is cut into launches of at most that many
        simulated minutes (whole steps) -- at 240 a wave costs 1.41 times its mean lane against 1.36 uncut, and a launch of
        1 Mi envs stays in the range of a second; the cut changes no result.  Per-env gains as in rollout_pid
        (t1d_rollout_pid_dopri5_gains)."""
        self._need_dopri5("rollout_pid_dopri5")
        gains = self._per_env_gains("rollout_pid_dopri5", P, I, D, target)
        if gains is None:
            pid_state, p = self._pid_struct(P, I, D, target, pid_state, stats)
            self._rollout_dopri5(self._L.t1d_rollout_pid_dopri5, p, n_steps, trace, max_minutes_per_launch)
        else:
            pid_state, p = self._pid_struct(0.0, 0.0, 0.0, 0.0, pid_state, stats)
            self._rollout_dopri5(self._L.t1d_rollout_pid_dopri5_gains, p, n_steps, trace, max_minutes_per_launch,
                                 extra=(C.byref(self._gains_struct(gains)),))
        return pid_state

    def rollout_bb_dopri5(self, n_steps, target=140.0, bb_state=None, stats=None, trace=None, max_minutes_per_launch=240):
        """rollout_bb in the exact mode (t1d_rollout_bb_dopri5): SimObj.simulate with BBController and scipy's dopri5 -- the
        reference's own regression run.  Arguments and return value as rollout_bb; h_carry, nfev and
        max_minutes_per_launch as in rollout_pid_dopri5."""
        self._need_dopri5("rollout_bb_dopri5")
        bb_state, p = self._bb_struct(target, bb_state, stats)
        self._rollout_dopri5(self._L.t1d_rollout_bb_dopri5, p, n_steps, trace, max_minutes_per_launch)
        return bb_state

    def model_rhs(self, x, patient_idx, cho, insulin, last_qsto, last_food, math=1):
        """T1DPatient.model (t1dpatient.py:119-208) at m independent points on the device: x [13, m], the others [m]
        (cho grams eaten in the minute, insulin U/min as the model takes it, i.e. without the pump) -> dx/dt [13, m].
        math = 0: ocml tanh / IEEE divisions as the reference writes them; 1: the step kernels' arithmetic."""
        t = lambda v, dt=self.dtype: torch.as_tensor(v, dtype=dt).to(self.device).contiguous()
        x = t(x); m = x.shape[1]
        if x.shape[0] != 13:
            raise ValueError("x must have shape [13, m]")
        pid = t(patient_idx, torch.int32); args = [t(v) for v in (cho, insulin, last_qsto, last_food)]
        if pid.shape != (m,) or any(v.shape != (m,) for v in args):
            raise ValueError("patient_idx, cho, insulin, last_qsto, last_food must have m entries")
        if m and (int(pid.min()) < 0 or int(pid.max()) >= len(self.names)):
            raise ValueError("patient_idx out of range for the context's table of %d patients" % len(self.names))
        out = torch.empty(13, m, dtype=self.dtype, device=self.device)
        p = lambda v: C.c_void_p(v.data_ptr())
        with torch.cuda.device(self.device):
            _lib.check(self._L.t1d_model_rhs(self._ctx, self._b.dtype, m, int(math), p(x), p(pid), p(args[0]), p(args[1]), p(args[2]),
                                             p(args[3]), p(out), self._stream()))
        return out

    def philox_normals(self, n_draws, draw0=0, episode=1):
        """The normals the kernels draw in Philox mode -> float64 [n_draws, n] (for replay tests)."""
        out = torch.empty(n_draws, self.n, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._L.t1d_philox_normals(self._ctx, self.seed, self.env_offset, self.n, int(episode),
                                                  int(draw0), int(n_draws), C.c_void_p(out.data_ptr()), self._stream()))
        return out

    def sync(self, raise_on_status=True):
        """Wait for the stream; -> status bits (T1D_ST_*)."""
        st = C.c_int32(0)
        with torch.cuda.device(self.device):
            rc = self._L.t1d_sync(self._ctx, self._stream(), C.byref(st))
        if rc != 0 and (raise_on_status or st.value == 0):
            _lib.check(rc)
        return st.value

    # ------------------------------------------------------------------ checkpoint
    STATE_FORMAT = 4           # = the ABI version whose state words the checkpoint holds (prev_risk, cgm0: since 3; dbar: 4)

    def state_dict(self):
        sd = {k: getattr(self, k).clone() for k in _STATE_KEYS + ("cgm", "cgm0")}
        sd["format"] = self.STATE_FORMAT
        if self.h_carry is not None:
            sd["h_carry"] = self.h_carry.clone()
        if self._hist is not None:
            sd.update({k: getattr(self, k).clone() for k in ("_hist", "_hist_pos", "_hist_cnt")})
        return sd

    def load_state_dict(self, sd):
        fmt = sd.get("format")
        if fmt != self.STATE_FORMAT or any(k not in sd for k in _STATE_KEYS + ("cgm", "cgm0")):
            raise _lib.T1DError("checkpoint format %r is not %d (checkpoints written before ABI 3 carry prev_cgm instead of "
                                "prev_risk and no cgm0, before ABI 4 no dbar): re-create it with this version" % (fmt, self.STATE_FORMAT))
        if self.h_carry is not None and "h_carry" not in sd:
            raise _lib.T1DError("an env with integrator='dopri5' needs the checkpoint's h_carry (the predicted step of every env): "
                                "take it from an env with integrator='dopri5'")
        for k in _STATE_KEYS + ("cgm", "cgm0"):
            getattr(self, k).copy_(sd[k])
        if self.h_carry is not None:
            self.h_carry.copy_(sd["h_carry"])
        if self._hist is not None:
            if all(k in sd for k in ("_hist", "_hist_pos", "_hist_cnt")):
                for k in ("_hist", "_hist_pos", "_hist_cnt"):
                    getattr(self, k).copy_(sd[k])
            else:
                # the checkpoint was taken without a CGM history: what the ring can honestly hold is the last observation
                self._hist_after_rollout()
        self._clock = None

    def close(self):
        if not self._closed and self._ctx:
            self._L.t1d_ctx_destroy(self._ctx)
            self._closed = True

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
