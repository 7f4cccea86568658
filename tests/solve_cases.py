"""The windows of tests/test_solve_hp.py and tests/test_step_hp.py: the smallest windows that still reach every part of the dense solve and
of the step half behind it (the reduced system is 172 x 172 whatever N is).  Built from lfvio.synth seeds; a case is built once per session
(window) and left unchanged.  CASES maps a name to (constructor(oracle) -> abi.Window, every mu of test_solve_hp?)."""
import numpy as np

from lfvio import abi, synth


def skip_imu0(w):
    imu = list(w.imu)
    big = abi.preint_from_array(abi.preint_to_array(imu[0]))
    big.sum_dt = 10.5  # > 10: the factor is skipped (estimator.cpp:720)
    imu[0] = big
    return w.copy(imu=imu)


def imu_only(oracle):
    w = synth.make_window(11, 1, estimate_extrinsic=0, estimate_td=0)
    return w.copy(start_frame=np.zeros(0, np.int32), obs_offset=np.zeros(1, np.int32), inv_depth=np.zeros(0), obs_point=np.zeros((0, 3)),
                  obs_velocity=np.zeros((0, 3)), obs_cur_td=np.zeros(0), obs_uv_y=np.zeros(0))


CASES = {
    "n64": (lambda o: synth.make_window(5, 64), True),             # one full landmark block
    "n65": (lambda o: synth.make_window(6, 65), False),            # one landmark past it
    "n7": (lambda o: synth.make_window(3, 7), True),               # nearly empty Schur sums: gauge directions held by mu D^2 alone
    "n1": (lambda o: synth.make_window(8, 1), False),
    "imu_only": (imu_only, False),                                # N = 0: C = 0 (ex and td constant: their columns would be zero)
    "prior": (lambda o: synth.make_window_with_prior(0, 64, o.optimize)[0], True),   # prior in H; the prior scatter of the assembling form
    "no_td": (lambda o: synth.make_window(5, 64, estimate_td=0), True),              # identity rows inside block column 4
    "no_ex": (lambda o: synth.make_window(5, 64, estimate_extrinsic=0), True),
    "no_td_no_ex": (lambda o: synth.make_window(5, 64, estimate_td=0, estimate_extrinsic=0), True),
    "static": (lambda o: synth.make_window(4, 64, motion="static", estimate_td=0), True),   # pivots crowded near mu D^2 (td: a zero column at rest)
    "rotate": (lambda o: synth.make_window(4, 64, motion="rotate"), True),
    "ocam_rs": (lambda o: synth.make_window(6, 120, camera="ocam", tr=0.02), False),  # a live td column with rolling shutter
    "skip_imu0": (lambda o: skip_imu0(synth.make_window_with_prior(9, 40, o.optimize)[0]), False),  # a zero 30 x 30 source in the assembly (the prior holds speed/bias 0)
    "bench": (lambda o: synth.make_window(0, 300), False),         # the shape the benchmark times: on the device once, in the batch
}
# The class of a case, known before anything is computed: (group, mu).  mu sets kappa_2(S), the unit of the forward metrics, which spans
# eight orders of magnitude over the four values.  Groups: "weak" — kappa_2(S) above 1e10 at the first mu (one landmark; speed/bias 0 held by
# the prior alone); "prior" — a prior puts entries of 1e5 and more into H beside the unit-sized ones, and the quadratic forms lose digits to
# cancellation in double in any order of evaluation; "regular" — everything else.
GROUP = {"n1": "weak", "skip_imu0": "weak", "prior": "prior"}


def case_class(name, mu):
    return (GROUP.get(name, "regular"), mu)


_win = {}


def window(oracle, name):
    if name not in _win:
        _win[name] = CASES[name][0](oracle)
    return _win[name]
