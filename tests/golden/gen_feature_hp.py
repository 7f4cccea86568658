"""Generates the 50-digit fixtures of the three feature steps (tests/hp_ref.py, mpmath) — inputs and expected outputs
rounded to double:

    python tests/golden/gen_feature_hp.py            # preint_hp.npz, triangulate_hp.npz, shift_hp.npz   (a few minutes)

The files are written with fixed zip time stamps, so a second run reproduces them bit for bit.  Every input comes from
np.random.default_rng with the seeds below (or from lfvio.synth, which is seeded the same way) and is stored in the file:
the GPU tests read the files alone.  case lists, loaders and the builders of single cases are importable
(tests/test_feature_hp.py re-runs a few small cases live).
"""
import io
import os
import sys
import zipfile
from concurrent.futures import ProcessPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "lf-vio_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
from lfvio import abi, synth  # noqa: E402

EPS = 2.0 ** -52
NOISE = [synth.ACC_N, synth.GYR_N, synth.ACC_W, synth.GYR_W]
NOISE2 = [1e-1, 1e-4, 1e-2, 1e-5]  # four magnitudes decades apart: a mixed-up entry of the noise diagonal shows

# ----------------------------------------------------------------------------------------------------------------
# pre-integration
# ----------------------------------------------------------------------------------------------------------------
PRE_N_USUAL = [1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 23, 24, 25, 31, 32, 33, 63, 64, 65, 200, 400]  # the issue's list and 3, 4: every n mod 8
PRE_N_EDGE = [7, 16, 33, 64, 400]
PRE_REGIMES = ["usual", "fast", "bias", "dt0_mid", "dt0_first", "noise0", "noise2"]


def pre_sample_set(kind, n):
    """(acc_0, gyr_0, dt[n], acc[n, 3], gyr[n, 3]) of sample set (kind, n): kind 0 the usual regime (dt uniform 2-8 ms,
    acc N(0, 3) + g, gyr N(0, 0.5)), kind 1 fast rotation (gyr sigma 8 rad/s)."""
    rng = np.random.default_rng([20241, kind, n])
    sg = 8.0 if kind == 1 else 0.5
    return (rng.normal(0, 3, 3) + [0, 0, 9.8], rng.normal(0, sg, 3), rng.uniform(0.002, 0.008, n),
            rng.normal(0, 3, (n, 3)) + [0, 0, 9.8], rng.normal(0, sg, (n, 3)))


def pre_case_list():
    """[(regime, n, set kind, noise, index of the dt == 0 sample or -1)] in stored order."""
    cases = [("usual", n, 0, NOISE, -1) for n in PRE_N_USUAL]
    for n in PRE_N_EDGE:
        T = (n + 7) // 8
        cases += [("fast", n, 1, NOISE, -1), ("bias", n, 0, NOISE, -1),
                  ("dt0_mid", n, 0, NOISE, 8 * ((T - 1) // 2) + 3),   # in mid-tile
                  ("dt0_first", n, 0, NOISE, 8 * (T // 2)),           # first sample of a tile (of the only one for n = 7)
                  ("noise0", n, 0, [0.0] * 4, -1), ("noise2", n, 0, NOISE2, -1)]
    return cases


def pre_case_biases(regime, n):
    rng = np.random.default_rng([20242, PRE_REGIMES.index(regime), n])
    s = (0.5, 0.1) if regime == "bias" else (0.05, 0.01)
    return rng.normal(0, s[0], 3), rng.normal(0, s[1], 3)


def pre_interval(case):
    """The interval of one case as Engine.preintegrate takes it: (ba, bg, acc_0, gyr_0, dt, acc, gyr)."""
    regime, n, kind, noise, zero = case
    a0, g0, dts, accs, gyrs = pre_sample_set(kind, n)
    if zero >= 0:
        dts = dts.copy()
        dts[zero] = 0.0
    ba, bg = pre_case_biases(regime, n)
    return ba, bg, a0, g0, dts, accs, gyrs


def pre_expected(case):
    import hp_ref

    ba, bg, a0, g0, dts, accs, gyrs = pre_interval(case)
    return hp_ref.preintegrate_array(hp_ref.preintegrate(a0, g0, ba, bg, dts, accs, gyrs, case[3]), ba, bg)


def gen_preint(pool):
    cases = pre_case_list()
    sets = sorted({(c[2], c[1]) for c in cases})
    data = [pre_sample_set(*s) for s in sets]
    off = np.concatenate([[0], np.cumsum([s[1] for s in sets])])
    ivs = [pre_interval(c) for c in cases]
    out = np.array(list(pool.map(pre_expected, cases)))
    return dict(set_kind=np.array([s[0] for s in sets]), set_n=np.array([s[1] for s in sets]), set_off=off,
                set_acc0=np.array([d[0] for d in data]), set_gyr0=np.array([d[1] for d in data]),
                set_dt=np.concatenate([d[2] for d in data]), set_acc=np.concatenate([d[3] for d in data]),
                set_gyr=np.concatenate([d[4] for d in data]),
                case_regime=np.array([c[0] for c in cases]), case_n=np.array([c[1] for c in cases]),
                case_set=np.array([sets.index((c[2], c[1])) for c in cases]), case_noise=np.array([c[3] for c in cases], dtype=float),
                case_zero=np.array([c[4] for c in cases]), case_ba=np.array([i[0] for i in ivs]),
                case_bg=np.array([i[1] for i in ivs]), case_out=out)


def load_preint(path):
    """[(test id, regime, n, noise[4], interval, expected[467])] from preint_hp.npz, stored order; nothing is regenerated."""
    d = np.load(path)
    res = []
    for k in range(len(d["case_n"])):
        s = int(d["case_set"][k])
        o0, o1 = int(d["set_off"][s]), int(d["set_off"][s + 1])
        dts = d["set_dt"][o0:o1].copy()
        if d["case_zero"][k] >= 0:
            dts[int(d["case_zero"][k])] = 0.0
        iv = (d["case_ba"][k], d["case_bg"][k], d["set_acc0"][s], d["set_gyr0"][s], dts, d["set_acc"][o0:o1], d["set_gyr"][o0:o1])
        regime, n = str(d["case_regime"][k]), int(d["case_n"][k])
        res.append((f"{regime}-n{n}", regime, n, d["case_noise"][k], iv, d["case_out"][k]))
    return res


# ----------------------------------------------------------------------------------------------------------------
# triangulation
# ----------------------------------------------------------------------------------------------------------------
TRI_MAX_COND = 1e8     # sigma_1 / sigma_4 of every stored landmark
TRI_SIGN_BAR = 1e3     # in units of eps sigma_1/sigma_4: no test bar of the suite may exceed it (asserted there)
TRI_LOW_PARALLAX = [1e-2, 1e-3, 1e-4]  # position noise [m] of the zero-baseline windows; none had to be enlarged


class _W:
    pass


def tri_input(g):
    """abi.TriangulateIn of a stored or freshly built group (dict with start_frame, obs_offset, obs_point, Ps, Rs, tic, ric)."""
    w = _W()
    w.start_frame, w.obs_offset, w.obs_point = g["start_frame"], g["obs_offset"], g["obs_point"]
    w.pose = np.zeros((abi.NUM_FRAMES, 7))
    w.pose[:, :3] = g["Ps"]
    w.ex_pose = np.zeros(7)
    w.ex_pose[:3] = g["tic"]
    return abi.TriangulateIn(w, Rs=g["Rs"], ric=g["ric"], init_depth=float(g["init_depth"]))


def _tri_group_of_window(w, depth_in, init_depth=5.0):
    tin = abi.TriangulateIn(w, init_depth=init_depth)
    return dict(start_frame=tin.start_frame, obs_offset=tin.obs_offset, obs_point=tin.obs_point, Ps=tin.Ps, Rs=tin.Rs,
                tic=tin.tic, ric=tin.ric, init_depth=np.float64(init_depth), depth_in=np.asarray(depth_in, float))


def _every_third_positive(n):
    d = -np.ones(n)
    d[::3] = 2.5 + 0.01 * np.arange(0, n, 3)
    return d


def _tri_all_pairs():
    """Every (start_frame s, track length k), k >= 2, s + k <= 11 twice (55 pairs), on the frames of make_window(5, 2): a point
    1-30 m away on the 40-120 degree annulus of the anchor camera, seen from frames s .. s + k - 1 with 1e-3 of bearing
    noise, bearings rounded through float32 as the window generator's are."""
    w = synth.make_window(5, 2)
    g = _tri_group_of_window(w, [])
    rng = np.random.default_rng(20243)
    Rc = [g["Rs"][f] @ g["ric"] for f in range(abi.NUM_FRAMES)]
    tc = [g["Ps"][f] + g["Rs"][f] @ g["tic"] for f in range(abi.NUM_FRAMES)]
    start, off, pts = [], [0], []
    for rep in range(2):
        for s in range(abi.NUM_FRAMES - 1):
            for k in range(2, abi.NUM_FRAMES - s + 1):
                th, ph, r = np.deg2rad(rng.uniform(40, 120)), rng.uniform(0, 2 * np.pi), rng.uniform(1.0, 30.0)
                X = tc[s] + Rc[s] @ (r * np.array([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)]))
                for j in range(s, s + k):
                    b = Rc[j].T @ (X - tc[j])
                    b = b / np.linalg.norm(b) + rng.normal(0, 1e-3, 3)
                    pts.append((b / np.linalg.norm(b)).astype(np.float32).astype(np.float64))
                start.append(s)
                off.append(off[-1] + k)
    g.update(start_frame=np.array(start, dtype=np.int32), obs_offset=np.array(off, dtype=np.int32), obs_point=np.array(pts),
             depth_in=-np.ones(len(start)))
    return g


def tri_groups():
    """{name: group inputs} in stored order."""
    gs = {}
    for name, (seed, n) in (("w0_300", (0, 300)), ("w3_60", (3, 60))):
        gs[name] = _tri_group_of_window(synth.make_window(seed, n), _every_third_positive(n))
    gs["pairs"] = _tri_all_pairs()
    for pn in TRI_LOW_PARALLAX:  # the camera does not translate and tic = 0: the position noise is the only baseline
        w = synth.make_window(3, 60, motion="rotate", pose_noise=(pn, np.deg2rad(0.5)))
        ex = w.ex_pose.copy()
        ex[:3] = 0.0
        gs[f"lowpar_{pn:g}"] = _tri_group_of_window(w.copy(ex_pose=ex), -np.ones(w.N))
    w = synth.make_window(4, 40)
    gs["mirror"] = _tri_group_of_window(w.copy(obs_point=-w.obs_point), -np.ones(w.N))
    return gs


def tri_expected_one(args):
    import hp_ref

    d, s, sc = hp_ref.triangulate_one(*args)
    return float(d), hp_ref.to_double(s), float(sc)


def tri_expected(g, pool=None, only=None):
    """depth_out, d_raw, sigma[N, 4], scale[N] of group g (landmarks `only`, default all)."""
    idx = range(len(g["start_frame"])) if only is None else only
    jobs = [(g["start_frame"][l], g["obs_point"][g["obs_offset"][l]:g["obs_offset"][l + 1]], g["Ps"], g["Rs"], g["tic"], g["ric"])
            for l in idx]
    res = list(pool.map(tri_expected_one, jobs, chunksize=8) if pool is not None else map(tri_expected_one, jobs))
    raw, sig, sc = np.array([r[0] for r in res]), np.array([r[1] for r in res]), np.array([r[2] for r in res])
    out = np.array(g["depth_in"], dtype=float)[list(idx)]
    fresh = ~(out > 0)
    out[fresh] = np.where(raw[fresh] >= 0, raw[fresh], float(g["init_depth"]))
    return out, raw, sig, sc


def gen_triangulate(pool):
    d, names = {}, []
    for name, g in tri_groups().items():
        out, raw, sig, sc = tri_expected(g, pool)
        cond = sig[:, 0] / sig[:, 3]
        assert cond.max() <= TRI_MAX_COND, (name, cond.max())  # enlarge the baseline of that family, do not drop landmarks
        margin = np.abs(raw) / (TRI_SIGN_BAR * EPS * cond * sc)
        assert margin.min() > 1e3, (name, margin.min())        # the sign of d is beyond every bar's reach
        print(f"triangulate {name}: {len(raw)} landmarks, sigma1/sigma4 {cond.min():.1e} .. {cond.max():.1e}, "
              f"{int((raw < 0).sum())} behind the camera, sign margin {margin.min():.1e} bars")
        names.append(name)
        for k, v in g.items():
            d[f"{name}.{k}"] = np.asarray(v)
        d[f"{name}.depth_out"], d[f"{name}.d_raw"], d[f"{name}.sigma"], d[f"{name}.scale"] = out, raw, sig, sc
    pairs = {(int(s), int(k)) for s, k in zip(d["pairs.start_frame"], np.diff(d["pairs.obs_offset"]))}
    assert len(pairs) == 55
    d["groups"] = np.array(names)
    return d


def load_triangulate(path):
    """{group: dict of its arrays} from triangulate_hp.npz."""
    d = np.load(path)
    return {str(n): {k[len(str(n)) + 1:]: d[k] for k in d.files if k.startswith(str(n) + ".")} for n in d["groups"]}


# ----------------------------------------------------------------------------------------------------------------
# shift depth
# ----------------------------------------------------------------------------------------------------------------
def _rot(rng, angle):
    return synth.exp_so3(rng.normal(0, angle, 3))


def shift_cases():
    """{name: dict(uv, marg_R, marg_P, new_R, new_P, init_depth, depth)}: sizes around the 256-thread group edge on ordinary
    poses, translations of ~1e3 m, a set whose sum nearly cancels, and depth 0 with marg_P == new_P (exactly 0)."""
    cs = {}

    def base(rng, n, far=1.0):
        uv = rng.normal(size=(n, 3))
        uv[:, 2] += 1.0
        uv /= np.linalg.norm(uv, axis=1)[:, None]
        mP = far * rng.normal(0, 1.0, 3)
        return dict(uv=uv, marg_R=_rot(rng, 0.5), marg_P=mP, new_R=_rot(rng, 0.5), new_P=mP + rng.normal(0, 0.3, 3),
                    init_depth=np.float64(5.0), depth=rng.uniform(0.5, 70.0, n))

    for n in (1, 255, 256, 257, 5000):
        cs[f"ordinary_n{n}"] = base(np.random.default_rng([20244, n]), n)
    cs["far_n257"] = base(np.random.default_rng([20245, 257]), 257, far=1e3)
    # near cancellation: the landmarks lie 1e-3 .. 1e-6 of |marg_P| + |depth uv| away from the new camera
    rng = np.random.default_rng([20246, 257])
    c = base(rng, 257)
    c["marg_P"], c["new_P"] = rng.normal(0, 10.0, 3), rng.normal(0, 10.0, 3)
    for l in range(257):
        dirn = rng.normal(size=3)
        terms = np.linalg.norm(c["new_P"] - c["marg_P"]) + np.linalg.norm(c["marg_P"]) + np.linalg.norm(c["new_P"])
        W = c["new_P"] + terms * 10.0 ** rng.uniform(-6, -3) * dirn / np.linalg.norm(dirn)
        p = c["marg_R"].T @ (W - c["marg_P"])
        c["depth"][l] = np.linalg.norm(p)
        c["uv"][l] = p / c["depth"][l]
    cs["cancel_n257"] = c
    c = base(np.random.default_rng([20247, 300]), 300)
    c["new_P"] = c["marg_P"].copy()
    c["depth"][::7] = 0.0
    c["depth"][[255, 256, 299]] = 0.0
    cs["zero_n300"] = c
    return cs


def shift_expected(c, only=None):
    import hp_ref

    sl = slice(None) if only is None else only
    return hp_ref.shift_depth(c["uv"][sl], c["marg_R"], c["marg_P"], c["new_R"], c["new_P"], c["init_depth"], c["depth"][sl])


def _shift_job(args):
    name, lo, hi = args
    return shift_expected(shift_cases()[name], slice(lo, hi))


def shift_args(c):
    return c["uv"], c["marg_R"], c["marg_P"], c["new_R"], c["new_P"], float(c["init_depth"]), c["depth"]


def gen_shift(pool):
    d, names = {}, []
    for name, c in shift_cases().items():
        n = len(c["depth"])
        out = np.concatenate(list(pool.map(_shift_job, [(name, lo, min(lo + 500, n)) for lo in range(0, n, 500)])))
        terms = np.abs(c["depth"]) * np.linalg.norm(c["uv"], axis=1) + np.linalg.norm(c["marg_P"]) + np.linalg.norm(c["new_P"])
        zero = (c["depth"] == 0) & np.array_equal(c["marg_P"], c["new_P"])
        assert np.array_equal(out[zero], np.full(int(zero.sum()), float(c["init_depth"])))
        ratio = out[~zero] / terms[~zero]
        print(f"shift {name}: range / terms {ratio.min():.1e} .. {ratio.max():.1e}, {int(zero.sum())} exact zeros")
        if name.startswith("cancel"):
            assert 0.9e-6 < ratio.min() and ratio.max() < 1.1e-3
        names.append(name)
        for k, v in c.items():
            d[f"{name}.{k}"] = np.asarray(v)
        d[f"{name}.out"] = out
    d["cases"] = np.array(names)
    return d


def load_shift(path):
    d = np.load(path)
    return {str(n): {k[len(str(n)) + 1:]: d[k] for k in d.files if k.startswith(str(n) + ".")} for n in d["cases"]}


# ----------------------------------------------------------------------------------------------------------------
def save_npz(path, arrays):
    """np.savez_compressed with fixed time stamps: the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k, v in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.require(v, requirements="C"), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED, 9)
    size = os.path.getsize(path)
    assert size <= 330 * 1024, (path, size)
    print(f"{os.path.basename(path)}: {size} bytes")


def main():
    with ProcessPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        save_npz(os.path.join(HERE, "shift_hp.npz"), gen_shift(pool))
        save_npz(os.path.join(HERE, "triangulate_hp.npz"), gen_triangulate(pool))
        save_npz(os.path.join(HERE, "preint_hp.npz"), gen_preint(pool))


if __name__ == "__main__":
    main()
