"""The float64 restatement of the convolution descriptor (tests/conv_replay.py) against the numpy emulator's nirgan_conv_igemm on every
distinct convolution launch the engines emit in a subset of scripts/plan_signature.py's configurations (plans built on CPU tensors under
the emulator, nothing of the nets runs): bitwise on integer data, within 2^-24 |ref| + 2^-40 scale on random data (the emulator contracts
in float64 too, in another order, then rounds to fp32), the statistics' and fused sums' records with it, and everything outside the written
sets still holding the sentinel.  The census alone has to show every feature of the descriptor the nets use (COVERAGE), and negative
controls show that the bitwise replay of tests/test_gpu_conv.py would notice a window off by one pixel or two taps swapped.  No GPU."""
import importlib.util
import os

import pytest
import torch

import conv_replay as R
from emu_pixel_disc import EmuPixelDisc
from nirgan_hip import lib as L
from nirgan_hip.options import OPT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("plan_signature", os.path.join(ROOT, "scripts", "plan_signature.py"))
P = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(P)

# the configurations whose census satisfies COVERAGE (small shapes first: the restatement and the emulator run on the host)
CONFIGS = ("g6_fp32_2x128_pad0", "g9_fp32_2x128_pad10", "g6_bf16_2x128_pad0", "g6_bf16x3_2x128_pad0", "inject", "no_fuse_inbwd_bf16_2x128",
           "no_epilogue_stats_bf16_2x128")
COVERAGE = {"in_stride 2", "out_stride 2", "in_oh", "out_oh", "run > in_cs", "ksplit > 1", "bias", "no bias", "precision 0", "precision 1",
            "precision 3", "in_bf16", "w_bf16", "out_bf16", "stats_ws", "fuse_y", "fuse_y_bf16", "out_span 2 (out_cs == N/2)",
            "out_span 2 (out_cs == N)", "group of 4", "N <= 64", "single", "group", "pair"}
# (no engine emits a descriptor with N % 4 != 0 -- the one-channel layers run on the endconv / tap kernels --: that feature is not in the set)

_CENSUS = {}


@pytest.fixture()
def emu():
    be = EmuPixelDisc()
    L.set_backend(be)
    yield be
    L.set_backend(None)
    OPT.reset()


def census(name):
    """the convolution launches of configuration `name` (copies of the descriptors; the engines are dropped).  The emulator is installed."""
    if name not in _CENSUS:
        zeros = torch.zeros
        torch.zeros = lambda *a, **kw: torch.empty(*a, **kw)       # building a plan reads no buffer (scripts/plan_signature.py)
        try:
            engines, keep = R.build_engines(P, P.CONFIGS[name])
            _CENSUS[name] = R.launches_of(engines, P.PLAN_NAMES)
            del engines, keep
        finally:
            torch.zeros = zeros
            OPT.reset()
    return _CENSUS[name]


def features(launch) -> set:
    seen = {launch.kind}
    if launch.kind == "group" and len(launch.ds) == 4:
        seen.add("group of 4")
    for d in launch.ds:
        seen.update({"in_stride 2"} if d.in_stride == 2 else set())
        seen.update({"out_stride 2"} if d.out_stride == 2 else set())
        seen.update({"in_oh"} if d.in_oh else set())
        seen.update({"out_oh"} if d.out_oh else set())
        seen.update({"run > in_cs"} if d.run > d.in_cs else set())
        seen.update({"ksplit > 1"} if d.ksplit > 1 else set())
        seen.add("bias" if d.bias else "no bias")
        seen.add(f"precision {d.precision}")
        for name in ("in_bf16", "w_bf16", "out_bf16", "stats_ws", "fuse_y", "fuse_y_bf16"):
            seen.update({name} if getattr(d, name) else set())
        if d.out_span == 2:
            seen.add("out_span 2 (out_cs == N)" if d.out_cs == d.N else "out_span 2 (out_cs == N/2)")
        seen.update({"N <= 64"} if d.N <= 64 else set())
        seen.update({"N % 4 != 0"} if d.N % 4 else set())
    return seen


def unique(launches, done=None):
    done, out = (set() if done is None else done), []
    for la in launches:
        k = la.geometry()
        if k not in done:
            done.add(k)
            out.append(la)
    return out


def emulate(emu, r: R.Replay):
    """the launch on the emulator, member by member (its group and pair entries do the same)"""
    r.arm()
    for f in r.members:
        assert emu.nirgan_conv_igemm(f.d) == 0, emu.nirgan_last_error()


def emu_bound(d, ref, scale):
    return 2.0 ** -24 * ref.abs() + 2.0 ** -40 * scale


def test_the_census_alone_covers_the_descriptor(emu):
    seen, count = set(), 0
    for name in CONFIGS:
        for la in census(name):
            seen |= features(la)
            count += 1
    print(f"\n{count} convolution launches in {len(CONFIGS)} configurations: {sorted(seen)}")
    assert COVERAGE <= seen, COVERAGE - seen


_DONE = set()       # geometries a previous configuration replayed


@pytest.mark.parametrize("config", CONFIGS)
def test_restatement_equals_the_emulator(emu, config):
    g = torch.Generator().manual_seed(5)
    todo = unique(census(config), _DONE)
    for la in todo:
        r = R.Replay(la, "cpu")
        for integers in (True, False):
            r.fill(integers, g)
            emulate(emu, r)
            r.verify(integers, emu_bound, f"{config}: {la.line()}")
    print(f"\n{config}: {len(census(config))} convolution launches, {len(todo)} geometries not replayed before")


# ------------------------------------------------------------------------------------------------------------ negative controls
def _first(pred):
    for name in CONFIGS:
        for la in census(name):
            for d in la.ds:
                if pred(d):
                    return d
    raise LookupError("no such descriptor in the census")


def _moved(d, **fields):
    m = R.copy_desc(d)
    for k, v in fields.items():
        setattr(m, k, v)
    return m


def _integer_restatement(d, f):
    return R.restate_conv(d, f.inp, f.w, f.bias, 0, kinds=("value",))


def _inside(d) -> bool:
    """the library's window checks (csrc/igemm_tiles.h::build_conv_params): such a descriptor would be accepted"""
    dh, dw = list(d.tap_dh[:d.ntaps]), list(d.tap_dw[:d.ntaps])
    return (d.in_oh + min(dh) >= 0 and (d.OH - 1) * d.in_stride + d.in_oh + max(dh) < d.in_hp and d.in_ow + min(dw) >= 0
            and ((d.OW - 1) * d.in_stride + d.in_ow + max(dw)) * d.in_cs + d.run <= d.in_wp * d.in_cs)


@pytest.mark.parametrize("field,delta", [("in_oh", 1), ("in_oh", -1), ("in_ow", 1), ("in_ow", -1)])
def test_an_input_window_off_by_one_changes_the_restatement(emu, field, delta):
    """on integer data (halos included) the restatement of a descriptor whose input window moved by one pixel differs from the unmoved one in
    most elements: the bitwise replay would notice.  The first descriptor of the census whose moved window stays inside its buffer."""
    d = _first(lambda d: not d.in_bf16 and d.ntaps >= 2 and _inside(_moved(d, **{field: getattr(d, field) + delta})))
    f = R.FreshConv(d, "cpu")
    g = torch.Generator().manual_seed(6)
    R._fill(f.inp, True, g)
    R._fill(f.w, True, g)
    _, (ref,) = _integer_restatement(f.d, f)
    _, (other,) = _integer_restatement(_moved(f.d, **{field: getattr(f.d, field) + delta}), f)
    assert (other != ref).double().mean() > 0.5


def test_two_taps_swapped_change_the_restatement(emu):
    d = _first(lambda d: not d.in_bf16 and d.ntaps >= 2 and d.tap_dh[0] != d.tap_dh[d.ntaps - 1])
    f = R.FreshConv(d, "cpu")
    g = torch.Generator().manual_seed(7)
    R._fill(f.inp, True, g)
    R._fill(f.w, True, g)
    _, (ref,) = _integer_restatement(f.d, f)
    m = R.copy_desc(f.d)
    last = m.ntaps - 1
    m.tap_dh[0], m.tap_dh[last] = m.tap_dh[last], m.tap_dh[0]
    assert _inside(m)
    _, (other,) = _integer_restatement(m, f)
    assert (other != ref).double().mean() > 0.5


def test_an_output_window_off_by_one_changes_the_restatement(emu):
    """out_ow + 1 with the window still inside the buffer: of the elements of `out` that either restatement writes, more than half get
    another value or are written by one of the two only"""
    room = lambda d: (d.OW - 1) * d.out_stride + d.out_ow + 1 + (R.span_of(d) - 1 if d.out_cs != d.N else 0) < d.out_wp      # noqa: E731
    d = _first(lambda d: not d.in_bf16 and room(d))
    f = R.FreshConv(d, "cpu")
    g = torch.Generator().manual_seed(8)
    R._fill(f.inp, True, g)
    R._fill(f.w, True, g)
    images = []
    for dd in (f.d, _moved(f.d, out_ow=f.d.out_ow + 1)):
        off, (val,) = _integer_restatement(dd, f)
        assert int(off.max()) < dd.out_elems
        img = torch.full((dd.out_elems,), float("nan"), dtype=torch.float64)
        img[off.reshape(-1)] = val.reshape(-1)
        images.append(img)
    a, b = images
    touched = ~(torch.isnan(a) & torch.isnan(b))
    same = (a == b)                      # (false where either is unwritten)
    assert (~same[touched]).double().mean() > 0.5


def test_the_replay_sees_a_stray_store_and_a_wrong_element(emu):
    """the checks themselves: one element outside the written set overwritten (a halo pixel, the guard, a record of another chunk) or one
    written element off by one is reported"""
    la = next(la for la in census(CONFIGS[0]) if la.kind == "group" and la.ds[0].stats_ws)
    r = R.Replay(la, "cpu")
    r.fill(True, torch.Generator().manual_seed(9))
    emulate(emu, r)
    r.verify(True, emu_bound, "untouched")
    f = r.members[0]
    for name, where in (("out", -1), ("stats_ws", -1)):
        saved = f.t[name][where].clone()
        f.t[name][where] = 1.0
        assert R.untouched(r.members, r.written) == [name]
        f.t[name][where] = saved
    written = set(r.written["out"].tolist())
    stray = next(i for i in range(f.d.out_elems + 1) if i not in written)   # (a halo pixel or one between the members' outputs, else the guard)
    f.out[stray] = 0.0
    with pytest.raises(AssertionError, match="outside the written set"):
        r.verify(True, emu_bound, "stray")
    emulate(emu, r)
    f.out[r.reference()[0]["off"][0, 0, 0]] += 1.0
    with pytest.raises(AssertionError, match="integer pass"):
        r.verify(True, emu_bound, "wrong")
