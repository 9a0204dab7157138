#!/usr/bin/env python3
"""Canonical signatures of the engines' launch plans, built on CPU tensors under the numpy emulator (nothing is launched).

For every configuration of CONFIGS a trainer (or a lone engine) is built and each engine's plans -- pack_fwd, fwd, pack_bwd, bwd,
bwd_frozen, bwd_pred, the discriminators' in_plan and the part plans the fused step asks for -- are written out as text: op names in
order, every positional argument, every field of every descriptor (nested arrays, the descriptors behind a group launch and the job
tables of the batched launches included).  An ADDRESS is replaced by the ordinal of its first appearance within the engine, so that buffer
sharing is part of the signature and the heap of the run is not; an address that is an index map (an int32 tensor the context keeps)
carries the CRC of the map.  What is an address is read from the ctypes field types of nirgan_hip/lib.py, for positional arguments from
lib.PROTOTYPES, for job tables from TABLE_ADDRESS_COLUMNS below.

tests/golden/plan_signatures.json holds, per (configuration, engine), the context's resident bytes and per plan the SHA-1 of that text
(with short per-op digests, so that tests/test_plan_signature.py can name the first op that differs).  A refactor of the host code must
leave the file byte-identical; a change that alters a plan on purpose regenerates it:

    python scripts/plan_signature.py            # compare with the fixture, print what differs
    python scripts/plan_signature.py --write    # regenerate the fixture
    python scripts/plan_signature.py --text base/G/bwd    # the canonical text of one plan
"""
import ctypes as C
import hashlib
import json
import os
import sys
import types
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "nir-gan_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)
FIXTURE = os.path.join(ROOT, "tests", "golden", "plan_signatures.json")

import torch  # noqa: E402

from nirgan_hip import lib as L  # noqa: E402
from nirgan_hip.engine import HOOK  # noqa: E402
from nirgan_hip.options import OPT  # noqa: E402

PLAN_NAMES = ("pack_fwd", "fwd", "pack_bwd", "bwd", "bwd_frozen", "bwd_pred", "in_plan")
PACK_OPS = ("nirgan_pack_rows", "nirgan_pack_rows_bf16", "nirgan_split3", "nirgan_wino6_weights_r", "nirgan_wino6_weights_x3")
# job tables in device memory (int64 rows): the columns that hold addresses (engine.Plan.fuse_packs / fuse_wino6_weights,
# engine.emit_deferred_reduce_rows)
TABLE_ADDRESS_COLUMNS = {"nirgan_pack_rows_batch": (0, 1, 2, 8), "nirgan_wino6_weights_batch": (0, 1, 7), "nirgan_reduce_rows_batch": (0, 1, 2)}


def _config(**kw):
    base = dict(blocks=6, precision="fp32", shape=(2, 128, 128), padding=0, netD="basic", inject=None, micro_batches=1, opt={}, infer=False)
    base.update(kw)
    return base


def _configs():
    out = {}
    # channel routing at ngf = 64: both depths, the three operand precisions, a small and an epilogue-sized shape, both paddings
    for prec in ("fp32", "bf16", "bf16x3"):
        for shape in ((2, 128, 128), (1, 256, 256)):
            for blocks, pad in ((6, 0), (9, 10)):
                out[f"g{blocks}_{prec}_{shape[0]}x{shape[1]}_pad{pad}"] = _config(blocks=blocks, precision=prec, shape=shape, padding=pad)
    out["rect_fp32_2x128x192"] = _config(shape=(2, 128, 192))              # a non-square tile
    out["rect_bf16_1x192x256"] = _config(shape=(1, 192, 256), precision="bf16")
    for pc in (False, True):
        inj = {"style": "multiply", "use_scale": True, "post_correction": pc}
        out["inject_pc_1x256_pad10" if pc else "inject"] = _config(blocks=9, inject=inj, **(dict(shape=(1, 256, 256), padding=10) if pc else {}))
    out["pixel_d"] = _config(netD="pixel")
    out["pixel_d_bf16_1x256"] = _config(netD="pixel", precision="bf16", shape=(1, 256, 256))
    out["infer_g9_pad10"] = _config(blocks=9, padding=10, infer=True)       # a need_backward=False GeneratorEngine
    out["infer_g6_bf16_1x256"] = _config(precision="bf16", shape=(1, 256, 256), infer=True)
    out["micro2"] = _config(micro_batches=2)
    out["micro2_bf16_2x256"] = _config(micro_batches=2, precision="bf16", shape=(2, 256, 256))
    for name in ("fold_apply", "fuse_inbwd", "fuse_dy_norm", "epilogue_stats", "batch_reduce", "pair_pixels", "split3"):
        out[f"no_{name}_fp32_1x256"] = _config(shape=(1, 256, 256), opt={name: False})
    for name in ("fuse_inbwd", "epilogue_stats", "batch_reduce", "bf16_y"):          # (what the bf16 operand mode routes differently)
        out[f"no_{name}_bf16_2x128"] = _config(precision="bf16", opt={name: False})
    out["winograd_off_1x256"] = _config(shape=(1, 256, 256), opt={"winograd": "off"})
    return out


CONFIGS = _configs()


# ---------------------------------------------------------------------------------------------- canonical text
class _Canon:
    """Addresses -> ordinals of first appearance, for one engine."""

    def __init__(self, ctx):
        self.ctx, self.ordinal = ctx, {}

    def _kept(self, dtype):
        return {t.data_ptr(): t for t in self.ctx.keep if isinstance(t, torch.Tensor) and t.dtype == dtype}

    def addr(self, a) -> str:
        if isinstance(a, C.c_void_p):
            a = a.value
        if not a:
            return "null"
        a = int(a)
        n = self.ordinal.setdefault(a, len(self.ordinal))
        imap = self._imaps.get(a)
        return f"@{n}" if imap is None else f"@{n}#{zlib.crc32(imap.numpy().tobytes()):08x}"

    def value(self, v) -> str:
        if isinstance(v, float):
            return repr(float(v))
        if isinstance(v, bytes):
            return repr(v)
        return str(int(v))

    def struct(self, s) -> str:
        parts = []
        for name, typ in s._fields_:
            v = getattr(s, name)
            if typ is C.c_void_p:
                parts.append(f"{name}={self.addr(v)}")
            elif issubclass(typ, C.Array):
                parts.append(f"{name}=[{','.join(self.value(x) for x in v)}]")
            elif issubclass(typ, (C._Pointer, C.Structure)):
                raise TypeError(f"{type(s).__name__}.{name}: nested pointer fields are not part of the engines' descriptors")
            else:
                parts.append(f"{name}={self.value(v)}")
        return f"{type(s).__name__}({' '.join(parts)})"

    def table(self, name, addr, rows) -> str:
        t = self._tables.get(int(addr))
        if t is None or t.shape[0] != rows:
            raise LookupError(f"{name}: job table not found among the context's tensors")
        cols = TABLE_ADDRESS_COLUMNS[name]
        return "[" + ";".join(",".join(self.addr(v) if j in cols else str(v) for j, v in enumerate(r)) for r in t.tolist()) + "]"

    def op(self, name, args) -> str:
        if name is HOOK:
            return "hook"
        protos = L.PROTOTYPES[name][1]
        assert len(args) == len(protos) - 1, (name, len(args), len(protos))       # (the stream is added by Plan.run)
        out = []
        for i, (a, typ) in enumerate(zip(args, protos)):
            if name in TABLE_ADDRESS_COLUMNS and i == 0:
                out.append(self.addr(a) + self.table(name, a, args[1]))
            elif isinstance(a, C.Array):
                if a._type_ is C.c_void_p:
                    out.append("[" + ",".join(self.addr(x) for x in a) + "]")
                else:
                    out.append("[" + ",".join(self.struct(x.contents) for x in a) + "]")
            elif hasattr(a, "_obj"):                  # ctypes.byref(descriptor)
                out.append(self.struct(a._obj))
            elif typ is C.c_void_p:
                out.append(self.addr(a))
            elif a is None:
                out.append("null")
            else:
                out.append(self.value(a))
        return f"{name}({', '.join(out)})"

    def plan(self, plan) -> list:
        if plan is None:
            return []
        self._imaps, self._tables = self._kept(torch.int32), self._kept(torch.int64)
        lines = [self.op(n, a) for n, a in plan.ops]
        if any(n in PACK_OPS for n, _ in plan.ops):
            # a pack plan runs in its batched form (nets._Engine.refresh_weights): signed as emitted AND as fused
            plan.fuse_packs()
            plan.fuse_wino6_weights()
            self._tables = self._kept(torch.int64)
            lines += ["-- fused"] + [self.op(n, a) for n, a in plan.ops]
        return lines


def _digest(lines):
    return hashlib.sha1("\n".join(lines).encode()).hexdigest()


def engine_signature(eng, part_plans=()) -> dict:
    """{"bytes": resident bytes of the context, "plans": {name: [canonical lines]}} of one engine."""
    canon = _Canon(eng.ctx)
    plans = {name: canon.plan(getattr(eng, name, None)) for name in PLAN_NAMES}
    for i, parts in enumerate(part_plans):
        plans[f"parts{i}"] = canon.plan(eng.input_plan(parts))
    return {"bytes": int(eng.ctx.bytes), "plans": plans}


# ---------------------------------------------------------------------------------------------- building
_NETS = {}


def _nets(cfg):
    """The two modules of a configuration (kept: their weights do not enter a plan, only where they live does)."""
    key = (cfg["blocks"], cfg["netD"], None if cfg["inject"] is None else bool(cfg["inject"].get("post_correction")))
    if key not in _NETS:
        _NETS[key] = _make_nets(cfg)
    return _NETS[key]


def _make_nets(cfg):
    from model import networks
    ns = types.SimpleNamespace
    nb = cfg["blocks"]
    if cfg["inject"] is not None:
        from model.generator_inject import define_G_inject
        pc = bool(cfg["inject"].get("post_correction"))
        netG = define_G_inject(ns(base_configs=ns(input_nc=3, output_nc=1, ngf=64, netG=f"resnet_{nb}blocks", norm="instance", no_dropout=True,
                                                  init_type="normal", init_gain=0.02),
                                  satclip=ns(satclip_inject_style="multiply", post_correction=pc, post_correction_init=0.8,
                                             scaling_param=True, scaling_param_init=0.01)))
    else:
        netG = networks.define_G(3, 1, 64, f"resnet_{nb}blocks", "instance", False, "normal", 0.02)
    netD = networks.define_D(4, 64, cfg["netD"], 3, "instance", "normal", 0.02)
    return netG, netD


def config_signature(cfg) -> dict:
    """{engine name: engine_signature} of one configuration.  The emulator must be installed (lib.set_backend)."""
    from nirgan_hip.nets import GeneratorEngine
    from nirgan_hip.trainer import Pix2PixTrainer
    OPT.reset()
    for k, v in cfg["opt"].items():
        assert hasattr(OPT, k), k
        setattr(OPT, k, v)
    try:
        netG, netD = _nets(cfg)
        B, H, W = cfg["shape"]
        if cfg["infer"]:
            flat = netG._flat()
            flat.ensure()
            eng = GeneratorEngine(flat.param_views(), None, cfg["blocks"], B, H, W, data_pad=cfg["padding"], inject=cfg["inject"],
                                  need_backward=False, precision=cfg["precision"])
            return {"G": engine_signature(eng)}
        tr = Pix2PixTrainer(netG, netD, n_blocks=cfg["blocks"], padding=cfg["padding"], inject=cfg["inject"], precision=cfg["precision"],
                            micro_batches=cfg["micro_batches"])
        tr._prepare(B, H, W)
        out = {}
        for i, m in enumerate(tr._state.micros):
            tag = f"m{i}." if tr._state.n > 1 else ""
            out[tag + "G"] = engine_signature(m.G)
            # the part plans of the fused step (trainer._d_pass / _g_pass)
            out[tag + "D2"] = engine_signature(m.D2, [[(m.rgb, 0, 0), (m.G.pred, 0, 3), (m.rgb, m.B, 0), (m.nir, m.B, 3)]])
            out[tag + "D1"] = engine_signature(m.D1, [[(m.rgb, 0, 0), (m.G.pred, 0, 3)]])
        return out
    finally:
        OPT.reset()


def all_signatures(names=None) -> dict:
    from emu_pixel_disc import EmuPixelDisc          # the emulator with every entry the engines ask for sizes
    L.set_backend(EmuPixelDisc())
    zeros = torch.zeros
    # building a plan reads no buffer: the engines' buffers are left untouched (a full-size generator is 1.7 GB of pages otherwise)
    torch.zeros = lambda *a, **kw: torch.empty(*a, **kw)
    try:
        return {name: config_signature(CONFIGS[name]) for name in (names or CONFIGS)}
    finally:
        torch.zeros = zeros
        L.set_backend(None)


def op_digest(line: str) -> str:
    return hashlib.sha1(line.encode()).hexdigest()[:6]


def fixture_of(sigs: dict) -> dict:
    """What is committed: per (configuration, engine) the bytes and per plan the SHA-1; the per-op digests once per distinct plan."""
    engines, ops = {}, {}
    for cname, engs in sigs.items():
        for ename, e in engs.items():
            rec = {"bytes": e["bytes"], "plans": {}}
            for pname, lines in e["plans"].items():
                sha = _digest(lines)
                rec["plans"][pname] = sha
                ops.setdefault(sha, "".join(op_digest(l) for l in lines))
            engines[f"{cname}/{ename}"] = rec
    return {"engines": engines, "ops": ops}


def compare(sigs: dict, fixture: dict) -> list:
    """Messages for everything in which `sigs` differs from the fixture; the first differing op of a plan is written out."""
    msgs = []
    have = fixture_of(sigs)["engines"]
    for key in sorted(set(have) | set(fixture["engines"])):
        if key.split("/")[0] not in sigs:
            continue
        new, old = have.get(key), fixture["engines"].get(key)
        if new is None or old is None:
            msgs.append(f"{key}: {'missing from the fixture' if old is None else 'no longer built'}")
            continue
        if new["bytes"] != old["bytes"]:
            msgs.append(f"{key}: resident bytes {new['bytes']} != {old['bytes']}")
        cname, ename = key.split("/")
        for pname in sorted(set(new["plans"]) | set(old["plans"])):
            a, b = new["plans"].get(pname), old["plans"].get(pname)
            if a == b:
                continue
            lines = sigs[cname][ename]["plans"].get(pname, [])
            was = fixture["ops"].get(b, "")
            was = [was[i:i + 6] for i in range(0, len(was), 6)]
            now = [op_digest(l) for l in lines]
            i = next((i for i, (x, y) in enumerate(zip(now, was)) if x != y), min(len(now), len(was)))
            what = lines[i] if i < len(lines) else "(the plan ends here)"
            msgs.append(f"{key}/{pname}: {len(now)} ops now, {len(was)} recorded; first difference at op {i}: {what}")
    return msgs


def main(argv):
    if "--text" in argv:
        cname, ename, pname = argv[argv.index("--text") + 1].split("/")
        print("\n".join(all_signatures([cname])[cname][ename]["plans"][pname]))
        return 0
    sigs = all_signatures()
    fx = fixture_of(sigs)
    for key, rec in fx["engines"].items():
        print(key, rec["bytes"], " ".join(f"{p}:{s[:10]}" for p, s in rec["plans"].items()))
    if "--write" in argv:
        with open(FIXTURE, "w") as f:
            json.dump(fx, f, indent=0, sort_keys=True)
            f.write("\n")
        print("wrote", FIXTURE)
        return 0
    with open(FIXTURE) as f:
        msgs = compare(sigs, json.load(f))
    print("\n".join(msgs) if msgs else "identical to the fixture")
    return 1 if msgs else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
