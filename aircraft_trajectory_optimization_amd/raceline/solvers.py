'''
Raceline solver classes with the reference's public surface (drone3d/raceline/*.py):

    GlobalDroneRaceline, ParametricDroneRaceline          drone_raceline.py:280-368
    GlobalPointRaceline, ParametricPointRaceline          point_raceline.py:48-74
    ParametricObstacleDroneRaceline, ParametricObstaclePointRaceline
                                                          drone_raceline.py:371-427, point_raceline.py:77-90

    solver = XxxRaceline(line, config, vehicle_config[, ...], ws_raceline=None, ws_model=None,
                         generate_ws=True)
    results: RacelineResults = solver.solve()          base_raceline.py:157-191
    solver.setup_time, solver.model, solver.ws_solver, solver.ws_raceline, solver.get_ws()

Instead of CasADi SX graphs and IPOPT, the constructor builds a ProblemSpec (host tables) and
a device evaluator over libato.so; solve() runs the interior-point solver (solver/ipm.py) whose
every g / J / f / grad f / Hessian evaluation runs in the HIP kernels. RacelineResults keeps the
reference's timing split: feval_time = time in device evaluation, ipopt_time = the rest.
'''
import time
from typing import Dict, List, Optional, Tuple

import numpy as np

from aircraft_trajectory_optimization_amd.centerlines.base_centerline import BaseCenterline
from aircraft_trajectory_optimization_amd.pytypes import DroneConfig, PointConfig
from aircraft_trajectory_optimization_amd.raceline.config import GlobalRacelineConfig, \
    ParametricRacelineConfig, RacelineConfig, RacelineResults
from aircraft_trajectory_optimization_amd.raceline.problem import ProblemSpec
from aircraft_trajectory_optimization_amd.utils.discretization_utils import interpolate_collocation, \
    interpolate_linear

# decision vectors of solutions produced here, so a RacelineResults can warm-start a drone solve
# further solver options for every solve (the reference passes ipopt.* options as a dict to
# ca.nlpsol, base_raceline.py:752-799): IPMOptions field names, e.g. {'max_soc': 0}
SOLVER_OPTIONS: dict = {}

_SOLUTIONS: Dict[int, Tuple[ProblemSpec, np.ndarray, RacelineResults]] = {}


def make_model(spec: ProblemSpec):
    ''' the dynamics model of a problem, as the reference's _get_model builds it
    (drone_raceline.py:314-316, :353-357; point_raceline.py:51-68) '''
    from aircraft_trajectory_optimization_amd.dynamics import DroneModel, ParametricDroneModel, \
        ParametricPointModel, PointModel
    if spec.is_drone:
        return ParametricDroneModel(spec.vehicle, spec.line) if spec.param else DroneModel(spec.vehicle)
    return ParametricPointModel(spec.vehicle, spec.line) if spec.param else PointModel(spec.vehicle)


class _Raceline:
    ''' shared machinery of every raceline solver '''
    frame = 'parametric'
    label = ''
    color: List[float] = [1, 1, 1, 1]
    sphere_table: Optional[np.ndarray] = None

    # evaluator over libato.so (tests substitute the CPU build of the programs here)
    evaluator_factory = None
    _last_solution = None

    def __init__(self, line: BaseCenterline, config: RacelineConfig, vehicle_config, ws_raceline=None,
                 ws_model=None, guess=None):
        t0 = time.time()
        factory = _Raceline.evaluator_factory
        if factory is None:
            from aircraft_trajectory_optimization_amd.raceline.evaluator import DeviceEvaluator as factory
        self.line, self.config, self.vehicle_config = line, config, vehicle_config
        self.ws_raceline, self.ws_model = ws_raceline, ws_model
        quat_flip, wraps = False, 0.0
        w_guess = None
        if guess is not None:
            w_guess, quat_flip, wraps = guess
        self.spec = ProblemSpec(line, config, vehicle_config, self.frame, quat_flip=quat_flip, euler_wraps=wraps,
                                sphere_table=self.sphere_table)
        if w_guess is not None:
            self.spec.w0, self.spec.lbw, self.spec.ubw = w_guess
        self.model = make_model(self.spec)
        self.evaluator = factory(self.spec)
        self.global_frame = not self.spec.param
        self.solve_time = self.ipopt_time = self.feval_time = 0.0
        self.result = None
        self.setup_time = time.time() - t0

    # ------------------------------------------------------------------ solving
    def solve(self) -> RacelineResults:
        from aircraft_trajectory_optimization_amd.raceline.evaluator import DeviceEvaluator
        from aircraft_trajectory_optimization_amd.solver.ipm import IPMOptions
        opts = IPMOptions(**{'max_iter': self.config.max_iter, 'verbose': bool(getattr(self.config, 'verbose', False)),
                             **SOLVER_OPTIONS})
        if isinstance(self.evaluator, DeviceEvaluator):
            x, success = self._solve_device(opts)
        else:
            x, success = self._solve_host(opts)
        self.ipopt_time = self.solve_time - self.feval_time
        out = self._unpack(x, success)
        _SOLUTIONS[id(out)] = (self.spec, x.copy(), out)
        self._last_solution = id(out)
        return out

    def _solve_device(self, opts):
        ''' the batched device solver at B = 1: evaluation, Hessian, KKT factorisation and solve all
        on the GPU (the host solver below factorises the KKT on the CPU) '''
        import torch
        from aircraft_trajectory_optimization_amd.solver.batched_ipm import device_solver
        sp_ = self.spec
        t0 = time.time()
        solver = device_solver(sp_, 1, sp_.lbw[None], sp_.ubw[None], opts)
        solver.ev.timing_on()
        res = solver.solve(sp_.w0[None])
        torch.cuda.synchronize()
        self.solve_time = time.time() - t0
        self.feval_time = solver.ev.timing_total_s()
        self.result = res
        return res.x[:, 0].cpu().numpy(), res.status[0] in ('optimal', 'acceptable')

    def _solve_host(self, opts):
        ''' the single-instance solver (host KKT) over the evaluator (the CPU build in tests) '''
        from aircraft_trajectory_optimization_amd.solver.ipm import InteriorPointSolver
        ev = self.evaluator
        ev.feval_time = 0.0
        solver = InteriorPointSolver(ev, self.spec.lbw, self.spec.ubw, ev.lbg, ev.ubg, opts)
        t0 = time.time()
        self.result = solver.solve(self.spec.w0)
        self.solve_time = time.time() - t0
        self.feval_time = ev.feval_time
        return self.result.x, self.result.success

    def replay(self, results_or_x=None, substeps: int = 16):
        '''
        Replay a solution of this problem through the vehicle dynamics on the device
        (raceline/replay.py): `results_or_x` is a RacelineResults of solve() (default: the last one)
        or a decision vector. Returns the ReplayResult of that one instance. Solver classes the
        replay does not cover (RK4 transcription, relative attitude) raise NotImplementedError.
        '''
        from aircraft_trajectory_optimization_amd.raceline.replay import replay_solutions
        return replay_solutions(self.spec, self._solution_vector(results_or_x)[None], substeps=substeps)

    def audit(self, results=None, samples: int = 16):
        '''
        Audit a solution of this problem between its collocation nodes on the device (raceline/audit.py):
        variable bounds, s' >= 0, regularity, the thrust ball and the ODE defects at samples + 1 points of
        every interval (samples = 0: the nodes). `results` is a RacelineResults of solve() (default: the last
        one) or a decision vector. Returns the AuditResult of that one instance, held to this problem's own
        bounds (where a bound differs between nodes, to the loosest of them). RK4 transcriptions raise
        NotImplementedError.
        '''
        from aircraft_trajectory_optimization_amd.raceline.audit import audit_solutions
        return audit_solutions(self.spec, self._solution_vector(results)[None], samples=samples, varying='outer')

    def gate_passage(self, results=None, samples: int = 16, tol: float = 0.0):
        '''
        Passage of a solution of this problem through its gates on the device (raceline/gates.py): where and when
        the continuous trajectory crosses each gate's plane and how far inside the opening. `results` is a
        RacelineResults of solve() (default: the last one) or a decision vector. Returns the GatePassageResult
        of that one instance. RK4 transcriptions raise NotImplementedError, a problem without gates (a
        parametric line without gate_s, a CPC problem) RuntimeError.
        '''
        from aircraft_trajectory_optimization_amd.raceline.gates import gate_passage
        return gate_passage(self.spec, self._solution_vector(results)[None], samples=samples, tol=tol)

    def _solution_vector(self, results_or_x=None) -> np.ndarray:
        ''' the decision vector of a RacelineResults of solve() (default: the last one), or the vector itself '''
        if results_or_x is None or isinstance(results_or_x, RacelineResults):
            key = id(results_or_x) if results_or_x is not None else self._last_solution
            if key not in _SOLUTIONS:
                raise ValueError('no decision vector is recorded for these results (call solve() first)')
            x = _SOLUTIONS[key][1]
        else:
            x = np.asarray(results_or_x, float).reshape(-1)
        if x.shape[0] != self.spec.nw:
            raise ValueError(f'decision vector of length {x.shape[0]}, problem has {self.spec.nw}')
        return x

    def refine(self, results=None, factor: int = 2, K: Optional[int] = None):
        '''
        A new solver of the same class on the refined discretisation (N * factor intervals of degree K,
        default the same K), seeded with the solution `results` (a RacelineResults of solve(), default
        the last one, or a decision vector) transferred to that mesh on the device (raceline/refine.py):
        .solve() warm-starts from it with h bounded to [h / 100, 10 h], .replay() certifies the result.
        RK4-transcribed problems (no collocation polynomial to transfer) and the obstacle classes (their
        tube tables depend on N) raise NotImplementedError.
        '''
        from aircraft_trajectory_optimization_amd.raceline.refine import refined_spec, transfer_solutions
        if self.spec.rk4:
            raise NotImplementedError('refine() does not cover RK4-transcribed racelines: there is no collocation '
                                      'polynomial to transfer')
        if self.spec.cpc is not None:
            raise NotImplementedError('refine() does not cover CPC problems: their progress variables are not a '
                                      'trajectory and are not transferred')
        if self.spec.sphere_table is not None or isinstance(self, _ObstacleMixin):
            raise NotImplementedError('refine() does not cover the obstacle racelines: their tube tables depend '
                                      'on N (build the finer problem and use raceline.refine.transfer_solutions)')
        x = self._solution_vector(results)
        dst = refined_spec(self.spec, factor, K)
        w0 = transfer_solutions(self.spec, x[None], dst)[:, 0].cpu().numpy()
        lbw, ubw = dst.lbw.copy(), dst.ubw.copy()
        lbw[:dst.N], ubw[:dst.N] = w0[:dst.N] / 100, w0[:dst.N] * 10
        # the constructor below builds its own spec from a copy of the refined config
        cfg = self.config.copy()
        cfg.N, cfg.K = dst.N, dst.K
        cfg.h0 = dst.config.h0
        new = object.__new__(type(self))
        _Raceline.__init__(new, self.line, cfg, self.vehicle_config, self.ws_raceline, self.ws_model,
                           guess=((w0, lbw, ubw), self.spec.quat_flip, self.spec.euler_wraps))
        if hasattr(self, 'ws_solver'):                   # the drone classes' point-mass warm-start solver
            new.ws_solver = self.ws_solver
        return new

    def get_ws(self) -> RacelineResults:
        ''' the initial guess, unpacked like a solution (base_raceline.py:193-198) '''
        return self._unpack(self.spec.w0, False)

    def _unpack(self, x, feasible) -> RacelineResults:
        ''' base_raceline.py:801-864 '''
        sp_ = self.spec
        N, K1, nz, nu = sp_.N, sp_.K1, sp_.nz, sp_.nu
        h = np.asarray(x[:N], float)
        t0 = np.concatenate([[0.0], np.cumsum(h)])[:-1]
        nodes = x[N:].reshape(N * K1, sp_.nv)
        Z, U, dU = nodes[:, :nz], nodes[:, nz:nz + nu], nodes[:, nz + nu:]
        states = []
        for n in range(N):
            for k in range(K1):
                i = n * K1 + k
                st = self.model.get_empty_state()
                st.t = float(t0[n] + sp_.tau[k] * h[n])
                self.model.zu2state(st, Z[i], U[i])
                self.model.du2state(st, dU[i])
                states.append(st)
        if sp_.rk4:
            zi, ui, dui = interpolate_linear(h, Z), interpolate_linear(h, U), interpolate_linear(h, dU)
        else:
            zi = interpolate_collocation(h, Z.reshape(N, K1, nz), sp_.K)
            ui = interpolate_collocation(h, U.reshape(N, K1, nu), sp_.K)
            dui = interpolate_collocation(h, dU.reshape(N, K1, nu), sp_.K)
        return RacelineResults(
            states=states, step_sizes=h, time=float(np.sum(h)), periodic=bool(self.config.closed),
            label=self.label, color=list(self.color), z_interp=zi, u_interp=ui, du_interp=dui,
            solve_time=self.solve_time, feval_time=self.feval_time, ipopt_time=self.ipopt_time,
            feasible=bool(feasible), global_frame=self.global_frame)


def _point_guess(solver_cls, line, config, vehicle_config: DroneConfig, generate_ws, ws_raceline, extra=()):
    ''' point-mass warm start: (ws_solver, ws_raceline, ws_model, drone guess builder) '''
    ws_solver = None
    if generate_ws:
        ws_config = config.copy()
        ws_config.verbose = False
        ws_config.plot_iterations = False
        point_config = PointConfig(global_r=vehicle_config.global_r,
                                   collision_radius=vehicle_config.collision_radius)
        print('Generating Warmstart... ')
        t0 = time.time()
        ws_solver = solver_cls(line, ws_config, point_config, *extra)
        ws_raceline = ws_solver.solve()
        print(f'Done (Lap Time: {ws_raceline.time:0.2f}s) (Setup + Solve: {time.time() - t0:0.2f}s)')
    if ws_raceline is None or id(ws_raceline) not in _SOLUTIONS:
        return ws_solver, ws_raceline, None, None
    pspec, x, _ = _SOLUTIONS[id(ws_raceline)]
    return ws_solver, ws_raceline, make_model(pspec), (pspec, x)


class _DroneRaceline(_Raceline):
    ''' drone racelines, optionally warm-started from a point-mass solve (drone_raceline.py:24-277) '''
    point_cls = None

    def __init__(self, line, config, vehicle_config: DroneConfig, ws_raceline=None, ws_model=None,
                 generate_ws: bool = True, extra=()):
        from aircraft_trajectory_optimization_amd.raceline.warmstart import drone_guess
        self.ws_solver, ws_raceline, pmodel, ws = _point_guess(self.point_cls, line, config, vehicle_config,
                                                               generate_ws, ws_raceline, extra)
        guess = None
        if ws is not None:
            # a provisional spec (on a copy of the config) gives the indexing and bounds
            prov = ProblemSpec(line, config.copy(), vehicle_config, self.frame, sphere_table=self.sphere_table)
            w0, lbw, ubw, flip, wraps = drone_guess(prov, ws[0], ws[1])
            guess = ((w0, lbw, ubw), flip, wraps)
        super().__init__(line, config, vehicle_config, ws_raceline, pmodel or ws_model, guess)


class GlobalPointRaceline(_Raceline):
    frame = 'global'
    label, color = 'Global PM', [1, 1, 1, 1]


class ParametricPointRaceline(_Raceline):
    frame = 'parametric'
    label, color = 'Parametric PM', [.5, .5, .5, 1]


class GlobalDroneRaceline(_DroneRaceline):
    frame = 'global'
    label, color = 'Global Drone', [0, 1, 0, 1]
    point_cls = GlobalPointRaceline

    def __init__(self, line, config: GlobalRacelineConfig, vehicle_config: DroneConfig, ws_raceline=None,
                 ws_model=None, generate_ws: bool = True):
        vehicle_config.global_r = True      # GlobalDroneRaceline._get_model (drone_raceline.py:314-316)
        super().__init__(line, config, vehicle_config, ws_raceline, ws_model, generate_ws)


class ParametricDroneRaceline(_DroneRaceline):
    frame = 'parametric'
    label, color = 'Parametric Drone', [1, 0, 0, 1]
    point_cls = ParametricPointRaceline

    def __init__(self, line, config: ParametricRacelineConfig, vehicle_config: DroneConfig, ws_raceline=None,
                 ws_model=None, generate_ws: bool = True):
        super().__init__(line, config, vehicle_config, ws_raceline, ws_model, generate_ws)


class _ObstacleMixin:
    ''' obstacle-tube rows and the post-solve collision check (base_raceline.py:1254-1327) '''

    def _setup_tube(self, line, config, vehicle_config, mesh_obstacle, tube):
        self.mesh_obstacle = mesh_obstacle
        self.tube = tube
        self.calc_tube_time = -1.0
        prov = ProblemSpec(line, config.copy(), vehicle_config, 'parametric')
        if self.tube is None:
            t0 = time.time()
            self.tube = mesh_obstacle.compute_plannning_tube(line, prov.node_s, vehicle_config.collision_radius)
            self.calc_tube_time = time.time() - t0
        self.sphere_table = self.tube.sphere_table(prov.node_s)

    def _after_setup(self):
        if self.calc_tube_time > 0:
            self.setup_time -= self.calc_tube_time

    def triangulate_setup_info(self, ubo=None) -> Dict[str, object]:
        ''' drawables of the obstacle-free tube (base_raceline.py:1329-1331) '''
        return self.tube.get_vertex_objects(ubo)

    def clearance(self, results=None, samples: int = 16):
        '''
        Clearance of a solution of this problem from the obstacle mesh (raceline/clearance.py): `results` is a
        RacelineResults of solve() (default: the last one) or a decision vector. samples = 0 is the node test
        _unpack prints; samples >= 1 also looks between the nodes. Returns the ClearanceResult of that one
        instance, judged at the vehicle's collision radius.
        '''
        from aircraft_trajectory_optimization_amd.raceline.clearance import clearance_solutions
        return clearance_solutions(self.spec, self._solution_vector(results)[None], self.mesh_obstacle,
                                   samples=samples, collision_radius=self.vehicle_config.collision_radius)

    def _unpack(self, x, feasible) -> RacelineResults:
        out = super()._unpack(x, feasible)
        xs = np.array([st.x.to_vec() for st in out.states])
        d = self.mesh_obstacle.signed_distance(xs)
        for st, dk in zip(out.states, d):
            st.d = float(dk)
        if getattr(self.config, 'verbose', False) and feasible:
            cr = self.vehicle_config.collision_radius
            verdict = 'Passed' if d.min() >= cr else 'Failed'
            print(f'{verdict} Collision Test (min: {d.min():0.3f}m, max: {d.max():0.3f}m, pass: {cr:0.3f}m)')
        return out


class ParametricObstaclePointRaceline(_ObstacleMixin, _Raceline):
    frame = 'parametric'
    label, color = 'PM w/ obstacles', [.3, .3, .3, 1]

    def __init__(self, line, config: ParametricRacelineConfig, vehicle_config: PointConfig, mesh_obstacle,
                 tube=None, ws_raceline=None, ws_model=None):
        self._setup_tube(line, config, vehicle_config, mesh_obstacle, tube)
        super().__init__(line, config, vehicle_config, ws_raceline, ws_model)
        self._after_setup()


class ParametricObstacleDroneRaceline(_ObstacleMixin, _DroneRaceline):
    frame = 'parametric'
    label, color = 'Drone w/ obstacles', [0, .3, 1, 1]
    point_cls = ParametricObstaclePointRaceline

    def __init__(self, line, config: ParametricRacelineConfig, vehicle_config: DroneConfig, mesh_obstacle,
                 tube=None, ws_raceline=None, ws_model=None, generate_ws: bool = True):
        if generate_ws:
            # the warm start computes the tube once; the drone reuses it (drone_raceline.py:376-410)
            ws_solver, ws_raceline, _, _ = _point_guess(ParametricObstaclePointRaceline, line, config,
                                                        vehicle_config, True, None, (mesh_obstacle,))
            tube = ws_solver.tube
            self._pre_ws = ws_solver
        self._setup_tube(line, config, vehicle_config, mesh_obstacle, tube)
        super().__init__(line, config, vehicle_config, ws_raceline, ws_model, generate_ws=False)
        if generate_ws:
            self.ws_solver = self._pre_ws
        self._after_setup()
