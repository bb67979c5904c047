"""Guard bands round every kernel entry point and the env step (tests/guard_util.py).

ONE table: a row is an entry point (or a pair that only makes sense together) and a generator of CASES; a case builds its pointer arguments from a seed -
every one an `Arg` with its role - and a `call` that launches on them.  A case runs three times: on plain exact-sized tensors, with every argument an
`aligned` banded view, and with every argument an `offset` one (natural alignment of the element type and no better; `place="aligned"` keeps single
arguments aligned: the cases with only ONE operand off 16 bytes, and the cases that step round a documented refusal).  After each banded run the bands are
checked, and the outputs must be the plain run's, bit for bit, but for

  * outputs summed by float atomics, which the project documents as not order-stable - the objective's loss, d_logstd and `stats`, the optimiser's `sq` and
    what follows from it: parameters and moments under a truncation coefficient below 1, the norm slots of the diagnostics record - held to the tolerance
    of their existing tests (`Arg.cmp`; the figures are named where they are defined).  ONE figure is new, because no existing test compares `sq` of
    two runs over several blocks: SQ_TOL, relative 2e-5 and no absolute part.  `sq` is the float atomic sum of at most 62 block partials here; two orders
    of that sum differ by at most 62 roundings of 2^-24 relative, 3.7e-6 - under the 2e-5 the optimiser's own tests grant what is computed from it;
  * an `offset` run that takes another instantiation because of an alignment branch (`Case.loose`): held to the tolerance of the entry's existing test
    against its reference (`Arg.alt`).  Each such case says which path it expects (`Case.path`);
  * a documented refusal (`Case.refuse`): the status is asserted and nothing may have been written.

The values themselves are pinned by the existing tests; nothing here restates a reference.  tests/test_guard_bands.py (no GPU) checks that every exported
function with a `stream` argument is covered here or is exempt with a reason.
"""
import ctypes as C

import pytest
import torch

import guard_util as gu
import parity_util as pu
from leibnizgym_amd import _capi as capi
from leibnizgym_amd import evaluate
from leibnizgym_amd import ppo_kernels as pk

DEV = "cuda:0"
F32, F64, I32, I64, U8, BOOL = torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8, torch.bool

# functions with a `stream` argument that have no row, each with its reason (tests/test_guard_bands.py: completeness)
EXEMPT = {
    "tfp_reset_state": "takes no caller buffer: it clears the library's own accumulators",
}
# the env step's entry points are the cells of test_env_step_through_banded_buffers, not rows of the table
STEP_ENTRY_POINTS = ("tf_step", "tf_step_random", "tf_reset", "tf_apply_resets", "tf_pre_step", "tf_simulate", "tf_post_step", "tf_finish_step")


class Arg:
    """one pointer argument.  role: gu.ROLES.  data: its contents (`in`, `inout`); shape / dtype: of an `out`.  cmp: how the banded run's result compares
    with the plain run's - "bits", (rtol, atol), a callable(got, want, what) or None (not compared).  alt: the same, used in the placements the case lists
    as `loose`.  place: "aligned" keeps this argument aligned in the `offset` run."""

    def __init__(self, name, role, data=None, shape=None, dtype=F32, cmp="bits", alt=None, full=True, finite=True, in_fill=0, place=None):
        assert (data is None) == (role == "out"), name
        self.name, self.role, self.data, self.cmp, self.alt, self.full, self.finite, self.in_fill, self.place = name, role, data, cmp, alt, full, finite, in_fill, place
        self.shape = tuple(data.shape) if data is not None else tuple(shape)
        self.dtype = data.dtype if data is not None else dtype


class Case:
    """args: [Arg]; call(t) -> status, t the dict name -> tensor; refuse: {placement: status} for documented refusals; loose: placements in which an
    alignment branch picks another instantiation; path: {placement: name} documents the path each placement is expected to take - documentation only, but
    for the walk rows, which assert their entry point through the library's call counts (pk.n_calls); after(t, handles): further assertions on a run"""

    def __init__(self, args, call, refuse=None, loose=(), path=None, after=None):
        self.args, self.call, self.refuse, self.loose, self.path, self.after = args, call, dict(refuse or {}), tuple(loose), dict(path or {}), after


class _Lib:
    """the trainer library, loaded at the first call (collecting this file needs no built library)"""

    def __getattr__(self, name):
        return getattr(pk.load(), name)


LIB = _Lib()


# ---- helpers of the builders ---------------------------------------------------------------------------------------------------------------------------
def _rng(seed):
    g = torch.Generator().manual_seed(int(seed))
    return (lambda *s: torch.randn(*s, generator=g)), (lambda *s: torch.rand(*s, generator=g)), g


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else t.data_ptr()


def _vp(ts):
    return (C.c_void_p * len(ts))(*[(_p(t)) for t in ts])


def _ip(vals):
    return (C.c_int32 * len(vals))(*[int(v) for v in vals])


def _close_scaled(rtol, atol_rel, atol):
    """the form of tests/test_ppo_kernels.py::test_mfma_linear_matches_torch_fp32: atol = atol_rel * max |want| + atol"""
    def cmp(got, want, what):
        torch.testing.assert_close(got, want, rtol=rtol, atol=atol_rel * float(want.abs().max()) + atol, msg=lambda m: f"{what}: {m}")
    return cmp


GEMM_ALT = _close_scaled(2e-5, 2e-5, 1e-6)          # test_mfma_linear_matches_torch_fp32
STATS_TOL = (2e-5, 1e-6)                            # test_fused_objective_matches_torch_fp32: loss and stats
DLS_TOL = (2e-4, 1e-7)                              # ... d_logstd
ADAM_TOL = (2e-5, 2e-7)                             # test_flat_clip_adam_matches_torch, test_optimiser_with_the_record_two_groups
SQ_TOL = (2e-5, 0.0)                                # NEW, see the module docstring: the optimiser's squared norms
DIAG_GN_REL = 2e-5                                  # test_ppo_diagnostics_gpu.py: the record's norm slots against the norms (pytest.approx rel)


# ---- per-layer products and their grouped forms --------------------------------------------------------------------------------------------------------
GEMM_SHAPES = [(3, 5, 7), (65, 100, 1), (64, 32, 64), (130, 200, 100), (77, 41, 33)]
CHUNK = 64                                          # rows per slab of tfp_gemm_tn_*: 130 and 77 rows are then three and two slabs, the last ragged


def _gemm_paths(K, off):
    """the instantiation each placement takes: the vector operand loads need K % 4 == 0 and both operands on 16 bytes"""
    vec = K % 4 == 0
    return dict(path={"plain": "vector" if vec else "scalar", "aligned": "vector" if vec else "scalar", "offset": "scalar"}, loose=("offset",) if vec else ())


def cases_linear_fwd():
    lib = LIB
    for M, K, N in GEMM_SHAPES:
        for off in ("all", "A", "W") if K % 4 == 0 else ("all",):
            def build(seed, M=M, K=K, N=N, off=off):
                r, _, _ = _rng(seed)
                act = 0 if N == 1 else 1
                args = [Arg("A", "in", r(M, K), place="aligned" if off == "W" else None), Arg("W", "in", r(N, K) * K ** -0.5, place="aligned" if off == "A" else None),
                        Arg("bias", "in", r(N)), Arg("C", "out", shape=(M, N), alt=GEMM_ALT)]
                return Case(args, lambda t: lib.tfp_linear_fwd(_p(t["A"]), _p(t["W"]), _p(t["bias"]), _p(t["C"]), M, N, K, act, _stream()), **_gemm_paths(K, off))
            yield f"{M}x{K}x{N}-off_{off}", build


def _nn_args(r, u, M, K, N, with_y, with_yout, off, yout_aligned):
    a = [Arg("A", "in", r(M, K), place="aligned" if off == "Y" else None), Arg("B", "in", r(K, N)), Arg("C", "out", shape=(M, N), alt=GEMM_ALT)]
    if with_y:
        a.append(Arg("Y", "in", u(M, K) - 0.3, place="aligned" if off == "A" else None))
    if with_yout:
        a.append(Arg("Yout", "in", u(M, N) - 0.3, place="aligned" if yout_aligned else None))
    return a


def cases_gemm_nn():
    lib = LIB
    for M, K, N in GEMM_SHAPES:
        for with_y, off in [(False, "all"), (True, "all")] + ([(True, "A"), (True, "Y")] if K % 4 == 0 else []):
            def build(seed, M=M, K=K, N=N, with_y=with_y, off=off):
                r, u, _ = _rng(seed)
                args = _nn_args(r, u, M, K, N, with_y, False, off, False)
                return Case(args, lambda t: lib.tfp_gemm_nn(_p(t["A"]), _p(t.get("Y")), _p(t["B"]), _p(t["C"]), M, N, K, _stream()), **_gemm_paths(K, off))
            yield f"{M}x{K}x{N}-{'Y' if with_y else 'noY'}-off_{off}", build


def cases_gemm_nn_dz():
    """Yout off 16 bytes with N % 4 == 0: -1 (include/trifinger_ppo.h), nothing launched; the same case with Yout kept aligned runs"""
    lib = LIB
    for M, K, N in GEMM_SHAPES:
        for with_y in (False, True):
            for yout_aligned in (False, True) if N % 4 == 0 else (False,):
                def build(seed, M=M, K=K, N=N, with_y=with_y, yout_aligned=yout_aligned):
                    r, u, _ = _rng(seed)
                    args = _nn_args(r, u, M, K, N, with_y, True, "all", yout_aligned)
                    kw = _gemm_paths(K, "all")
                    refuse = {"offset": -1} if (N % 4 == 0 and not yout_aligned) else None
                    if refuse:
                        kw["path"]["offset"], kw["loose"] = "refusal", ()
                    return Case(args, lambda t: lib.tfp_gemm_nn_dz(_p(t["A"]), _p(t.get("Y")), _p(t["B"]), _p(t["Yout"]), _p(t["C"]), M, N, K, _stream()),
                                refuse=refuse, **kw)
                yield f"{M}x{K}x{N}-{'Y' if with_y else 'noY'}-Yout{'_aligned' if yout_aligned else ''}", build


def _tn_args(r, u, M, K, N, with_y, tag=""):
    """weight / bias gradient of the layer (M, K, N): dZ [M, N], the layer input [M, K] -> gw [N, K], gb [N]; the slabs in `part`"""
    splits = (M + CHUNK - 1) // CHUNK
    a = [Arg("A" + tag, "in", r(M, N)), Arg("B" + tag, "in", r(M, K)), Arg("part" + tag, "out", shape=(splits, N, K + 1))]
    if with_y:
        a.append(Arg("Y" + tag, "in", u(M, N) - 0.3))
    return a, splits


def cases_gemm_tn_bias():
    lib = LIB
    for M, K, N in GEMM_SHAPES:
        for with_y in (False, True):
            def build(seed, M=M, K=K, N=N, with_y=with_y):
                r, u, _ = _rng(seed)
                args, _ = _tn_args(r, u, M, K, N, with_y)
                args += [Arg("gw", "out", shape=(N, K)), Arg("gb", "out", shape=(N,))]
                return Case(args, lambda t: lib.tfp_gemm_tn_bias(_p(t["A"]), _p(t.get("Y")), _p(t["B"]), _p(t["part"]), _p(t["gw"]), _p(t["gb"]), M, N, K, CHUNK,
                                                                 _stream()), path={"offset": "scalar (the only one)"})
            yield f"{M}x{K}x{N}-{'Y' if with_y else 'noY'}", build


def cases_gemm_tn_partials():
    """the chunk products alone, then tfp_sum_partials_multi of one layer into gw / gb"""
    lib = LIB
    for M, K, N in GEMM_SHAPES:
        def build(seed, M=M, K=K, N=N):
            r, u, _ = _rng(seed)
            args, splits = _tn_args(r, u, M, K, N, True)
            args += [Arg("gw", "out", shape=(N, K)), Arg("gb", "out", shape=(N,))]

            def call(t):
                rc = lib.tfp_gemm_tn_partials(_p(t["A"]), _p(t["Y"]), _p(t["B"]), _p(t["part"]), M, N, K, CHUNK, _stream())
                return rc or lib.tfp_sum_partials_multi(_vp([t["part"]]), _vp([t["gw"]]), _vp([t["gb"]]), _ip([splits]), _ip([N]), _ip([K]), 1, _stream())
            return Case(args, call, path={"offset": "scalar (the only one)"})
        yield f"{M}x{K}x{N}", build


# pairs of one alignment class: both scalar (K % 4 != 0), both vector
GROUP_PAIRS = {"scalar": [(77, 41, 33), (3, 5, 7)], "vector": [(64, 32, 64), (130, 200, 100)], "vector_col": [(65, 100, 1), (64, 32, 64)]}


def _group_kw(kind, mixed):
    """all problems offset: every one takes the scalar loads; problem 0 kept aligned: mixed alignment classes, -4 and nothing launched"""
    if kind == "scalar":
        return dict(path={"plain": "scalar", "aligned": "scalar", "offset": "scalar"})
    if mixed:
        return dict(path={"plain": "vector", "aligned": "vector", "offset": "refusal"}, refuse={"offset": -4})
    return dict(path={"plain": "vector", "aligned": "vector", "offset": "scalar"}, loose=("offset",))


def cases_linear_fwd_group():
    lib = LIB
    for kind, shapes in GROUP_PAIRS.items():
        for mixed in (False, True) if kind != "scalar" else (False,):
            def build(seed, shapes=shapes, kind=kind, mixed=mixed):
                r, _, _ = _rng(seed)
                args = []
                for i, (M, K, N) in enumerate(shapes):
                    pl = "aligned" if (mixed and i == 0) else None
                    args += [Arg(f"A{i}", "in", r(M, K), place=pl), Arg(f"W{i}", "in", r(N, K) * K ** -0.5, place=pl), Arg(f"b{i}", "in", r(N)),
                             Arg(f"C{i}", "out", shape=(M, N), alt=GEMM_ALT)]
                n = len(shapes)

                def call(t):
                    return lib.tfp_linear_fwd_group(_vp([t[f"A{i}"] for i in range(n)]), _vp([t[f"W{i}"] for i in range(n)]), _vp([t[f"b{i}"] for i in range(n)]),
                                                    _vp([t[f"C{i}"] for i in range(n)]), _ip([s[0] for s in shapes]), _ip([s[2] for s in shapes]),
                                                    _ip([s[1] for s in shapes]), 1, n, _stream())
                return Case(args, call, **_group_kw(kind, mixed))
            yield f"{kind}{'-mixed' if mixed else ''}", build


def cases_gemm_nn_group(dz):
    lib = LIB
    for kind, shapes in GROUP_PAIRS.items():
        for with_y in (False, True):
            for mixed in (False, True) if kind != "scalar" else (False,):
                def build(seed, shapes=shapes, kind=kind, with_y=with_y, mixed=mixed):
                    r, u, _ = _rng(seed)
                    args = []
                    for i, (M, K, N) in enumerate(shapes):
                        pl = "aligned" if (mixed and i == 0) else None
                        args += [Arg(f"A{i}", "in", r(M, K), place=pl), Arg(f"B{i}", "in", r(K, N)), Arg(f"C{i}", "out", shape=(M, N), alt=GEMM_ALT)]
                        if with_y:
                            args.append(Arg(f"Y{i}", "in", u(M, K) - 0.3, place=pl))
                        if dz:                                                     # kept aligned: the refusal of a misaligned Yout is tfp_gemm_nn_dz's row
                            args.append(Arg(f"E{i}", "in", u(M, N) - 0.3, place="aligned"))
                    n = len(shapes)

                    def call(t):
                        A, B, Cs = _vp([t[f"A{i}"] for i in range(n)]), _vp([t[f"B{i}"] for i in range(n)]), _vp([t[f"C{i}"] for i in range(n)])
                        Y = _vp([t[f"Y{i}"] for i in range(n)]) if with_y else None
                        dims = (_ip([s[0] for s in shapes]), _ip([s[2] for s in shapes]), _ip([s[1] for s in shapes]))
                        if dz:
                            return lib.tfp_gemm_nn_dz_group(A, Y, B, _vp([t[f"E{i}"] for i in range(n)]), Cs, *dims, n, _stream())
                        return lib.tfp_gemm_nn_group(A, Y, B, Cs, *dims, n, _stream())
                    return Case(args, call, **_group_kw(kind, mixed))
                yield f"{kind}-{'Y' if with_y else 'noY'}{'-mixed' if mixed else ''}", build


def cases_gemm_tn_partials_group():
    lib = LIB
    for kind, shapes in GROUP_PAIRS.items():
        for with_y in (False, True):
            def build(seed, shapes=shapes, with_y=with_y):
                r, u, _ = _rng(seed)
                args, splits = [], []
                for i, (M, K, N) in enumerate(shapes):
                    a, sp = _tn_args(r, u, M, K, N, with_y, tag=str(i))
                    args += a + [Arg(f"gw{i}", "out", shape=(N, K)), Arg(f"gb{i}", "out", shape=(N,))]
                    splits.append(sp)
                n = len(shapes)

                def call(t):
                    ls = lambda k: [t[f"{k}{i}"] for i in range(n)]                                          # noqa: E731
                    rows, n1, n2 = _ip([s[0] for s in shapes]), _ip([s[2] for s in shapes]), _ip([s[1] for s in shapes])
                    rc = lib.tfp_gemm_tn_partials_group(_vp(ls("A")), _vp(ls("Y")) if with_y else None, _vp(ls("B")), _vp(ls("part")), rows, n1, n2, CHUNK, n,
                                                        _stream())
                    return rc or lib.tfp_sum_partials_multi(_vp(ls("part")), _vp(ls("gw")), _vp(ls("gb")), _ip(splits), n1, n2, n, _stream())
                return Case(args, call, path={"offset": "scalar (the only one)"})
            yield f"{kind}-{'Y' if with_y else 'noY'}", build


# ---- the direct weight gradients: the outputs are slots of ONE flat buffer laid out as FlatClipAdam lays it out ------------------------------------------
DW_SHAPES = [(9, 100), (1, 100), (64, 64), (65, 63), (400, 41), (17, 128)]      # (N1, N2); N2 = 64 and 128: the bias column alone in a block, 63: last in one


def _flat_layout(shapes):
    """FlatClipAdam's: every parameter - weight [N1, N2], then bias [N1] - starts on a multiple of four floats; -> [(gw offset, gb offset)], total"""
    al = lambda n: (n + 3) & ~3                                                                            # noqa: E731
    off, out = 0, []
    for n1, n2 in shapes:
        gw = off
        off += al(n1 * n2)
        out.append((gw, off))
        off += al(n1)
    return out, off


def cases_gemm_tn_partials_direct(bf16):
    lib = LIB
    entry = "tfp_gemm_tn_partials_direct_bf16" if bf16 else "tfp_gemm_tn_partials_direct"
    for rows in (77, 1100):                                          # less than a slab; two slabs, the second ragged
        def build(seed, rows=rows):
            r, _, _ = _rng(seed)
            chunk = lib.tfp_gemm_tn_partials_direct_chunk()
            splits = (rows + chunk - 1) // chunk
            slots, total = _flat_layout(DW_SHAPES)
            args = [Arg("flat_g", "out", shape=(total,), full=False)]                 # the padding floats of the layout are never written
            for i, (n1, n2) in enumerate(DW_SHAPES):
                args += [Arg(f"A{i}", "in", r(rows, n1)), Arg(f"B{i}", "in", r(rows, n2)), Arg(f"part{i}", "out", shape=(splits, n1, n2 + 1))]
            n = len(DW_SHAPES)

            def views(t):
                g = t["flat_g"]
                return [g[a:a + n1 * n2] for (a, _), (n1, n2) in zip(slots, DW_SHAPES)], [g[b:b + n1] for (_, b), (n1, _) in zip(slots, DW_SHAPES)]

            def call(t):
                ls = lambda k: [t[f"{k}{i}"] for i in range(n)]                                            # noqa: E731
                n1, n2 = _ip([s[0] for s in DW_SHAPES]), _ip([s[1] for s in DW_SHAPES])
                rc = getattr(lib, entry)(_vp(ls("A")), _vp(ls("B")), _vp(ls("part")), _ip([rows] * n), n1, n2, n, _stream())
                gw, gb = views(t)
                return rc or lib.tfp_sum_partials_multi(_vp(ls("part")), _vp(gw), _vp(gb), _ip([splits] * n), n1, n2, n, _stream())

            def after(t, handles):
                """every slot fully written, every padding float between two slots untouched: a slot's neighbours are its bands"""
                bits = t["flat_g"].view(I32)
                written = torch.zeros(total, dtype=BOOL, device=bits.device)
                for (a, b), (n1, n2) in zip(slots, DW_SHAPES):
                    written[a:a + n1 * n2] = True
                    written[b:b + n1] = True
                sentinel = bits == gu.OUT_NAN_F32
                assert not bool((sentinel & written).any()), f"unwritten gradient element at flat offset {int(torch.nonzero(sentinel & written)[0, 0])}"
                assert bool(sentinel[~written].all()), f"padding written at flat offset {int(torch.nonzero(~sentinel & ~written)[0, 0])}"
            return Case(args, call, after=after, path={"offset": "the one instantiation: buffer loads of operands off 16 bytes"})
        yield f"rows{rows}", build


# ---- the network walk ------------------------------------------------------------------------------------------------------------------------------------
WALK_SHAPES = [(77, [7, 33, 64, 5], [20, 416, 17, 3]), (64, [16, 16], [3, 1]), (33, [41, 48, 20, 9], None)]
WALK_KINDS = {
    # kind: (forward entry, backward entry, extended, mixed)
    "plain": ("tfp_mlp_forward", "tfp_mlp_backward", False, False),
    "stats": ("tfp_mlp_forward_norm", None, False, False),
    "ext": ("tfp_net_forward", "tfp_net_backward", True, False),
    "bf16": ("tfp_net_forward_bf16", "tfp_net_backward_bf16", True, True),
}


def _walk_nets(r, u, M, dims_list, kind, stats_for=(0,)):
    """-> [(x, [(w, b, act)], d2rl, stats)] on the host; `ext` / `bf16`: activation codes 2 .. 6 in turn, d2rl where the network has a wide layer; statistics
    for the networks `stats_for` (not for the plain kind)"""
    ext = WALK_KINDS[kind][2]
    nets = []
    for ni, dims in enumerate(d for d in dims_list if d is not None):
        n = len(dims) - 1
        d2rl = ext and n >= 3 and ni == 0
        layers = []
        for i in range(n):
            kin = dims[i] + (dims[0] if (d2rl and 1 <= i <= n - 2) else 0)
            act = 0 if i == n - 1 else ((2 + (i + ni) % 5) if ext else 1)
            layers.append((r(dims[i + 1], kin) * kin ** -0.5, r(dims[i + 1]) * 0.3, act))
        stats = (r(dims[0]) * 0.5, u(dims[0]) + 0.5, 5.0) if (kind != "plain" and ni in stats_for) else None
        nets.append((r(M, dims[0]), layers, d2rl, stats))
    return nets


def _walk_layerlist(t, ni, layers, d2rl, mixed):
    ll = pk.LayerList([(t[f"W{ni}_{l}"], t[f"b{ni}_{l}"], act, None) for l, (_, _, act) in enumerate(layers)])
    ll.d2rl, ll.mixed = d2rl, mixed
    return ll


# tfp_mlp_forward_norm at the rows and input widths of the running moments: one row, just under a wavefront, sixteen row blocks and a ragged one of one row;
# widths 1, 41 and 113 (113: the critic's, ragged in K); in the pairs BOTH networks carry statistics
NORM_WALK_SHAPES = [(rows, da, dc) for rows in (1, 63, 1025) for da, dc in (([1, 33, 5], None), ([41, 48, 20, 9], [113, 64, 3]), ([113, 48, 9], [1, 16, 1]))]


def cases_walk(kind, direction, shapes=WALK_SHAPES, stats_for=(0,)):
    fwd_name, bwd_name, ext, mixed = WALK_KINDS[kind]
    name = fwd_name if direction == "forward" else bwd_name
    for M, dims_a, dims_c in shapes:
        for store_hidden in (True, False) if direction == "forward" else (True,):
            def build(seed, M=M, dims=(dims_a, dims_c), store_hidden=store_hidden):
                r, u, _ = _rng(seed)
                nets = _walk_nets(r, u, M, dims, kind, stats_for)
                args = []
                for ni, (x, layers, d2rl, stats) in enumerate(nets):
                    n = len(layers)
                    d0 = layers[0][0].shape[1]
                    width = lambda l: layers[l][0].shape[0] + (d0 if (d2rl and l <= n - 3) else 0)                 # noqa: E731
                    for l, (w, b, _) in enumerate(layers):
                        args += [Arg(f"W{ni}_{l}", "in", w), Arg(f"b{ni}_{l}", "in", b)]
                    if stats is not None and direction == "forward":
                        args += [Arg(f"mean{ni}", "in", stats[0]), Arg(f"inv{ni}", "in", stats[1])]
                    if direction == "forward":
                        args.append(Arg(f"x{ni}", "in", x))
                        args += [Arg(f"y{ni}_{l}", "out", shape=(M, width(l))) for l in range(n) if (store_hidden or l == n - 1)]
                    else:                                   # saved outputs in the range of their activation would need a forward: any finite rows serve
                        args.append(Arg(f"gy{ni}", "in", r(M, layers[-1][0].shape[0])))
                        args += [Arg(f"ys{ni}_{l}", "in", (u(M, width(l)) - 0.3) * 0.9) for l in range(n - 1)]
                        args += [Arg(f"dz{ni}_{l}", "out", shape=(M, layers[l][0].shape[0])) for l in range(n - 1)]

                def call(t):
                    before = pk.n_calls.get(name, 0)
                    lls = [_walk_layerlist(t, ni, layers, d2rl, mixed) for ni, (_, layers, d2rl, _) in enumerate(nets)]
                    if direction == "forward":
                        norms = [(t[f"mean{ni}"], t[f"inv{ni}"], st[2]) if st is not None else None for ni, (_, _, _, st) in enumerate(nets)]
                        outs = [[t.get(f"y{ni}_{l}") for l in range(len(layers))] for ni, (_, layers, _, _) in enumerate(nets)]
                        got = pk.mlp_walk_forward([(t[f"x{ni}"], ll) for ni, ll in enumerate(lls)], store_hidden, norms if kind != "plain" else None,
                                                  ext=ext, mixed=mixed, outs=outs)
                    else:
                        outs = [[t[f"dz{ni}_{l}"] for l in range(len(layers) - 1)] for ni, (_, layers, _, _) in enumerate(nets)]
                        ys = [[t[f"ys{ni}_{l}"] for l in range(len(layers) - 1)] + [t[f"gy{ni}"]] for ni, (_, layers, _, _) in enumerate(nets)]
                        got = pk.mlp_walk_backward([(t[f"gy{ni}"], ys[ni], ll) for ni, ll in enumerate(lls)], ext=ext, mixed=mixed, outs=outs)
                    assert got is not None, "the walk declined shapes its own test runs"
                    assert pk.n_calls.get(name, 0) == before + 1, f"{name} was not the entry point taken"
                    return 0
                return Case(args, call, path={"offset": f"{name}: weights by buffer loads off 16 bytes; pending rows element by element where the walk streams them out"})
            yield f"M{M}-in{dims_a[0]}{'' if dims_c is None else '_' + str(dims_c[0])}-{len(dims_a) - 1}layers{'' if store_hidden else '-last_only'}", build


# ---- gathers --------------------------------------------------------------------------------------------------------------------------------------------
GATHER_WIDTHS, GATHER_SRC_ROWS = (41, 9, 113, 1), 300


def _gather_idx(rows, g):
    """repeats, and both ends of the source"""
    idx = torch.randint(0, GATHER_SRC_ROWS, (rows,), generator=g, dtype=I64)
    idx[0] = GATHER_SRC_ROWS - 1
    if rows > 1:
        idx[-1] = 0
    if rows > 3:
        idx[2] = idx[1]
    return idx


def _sym_table(w, g):
    """a table of include/trifinger_ppo_symmetry.h for a w-wide array: 2 w entries {ia, ib, ca, cb}, 0 <= ia, ib < w, cb == 0 for every other column"""
    t = torch.zeros(2, w, 4, dtype=I32)
    t[..., 0] = torch.stack([torch.randperm(w, generator=g), torch.randperm(w, generator=g)]).to(I32)
    t[..., 1] = torch.stack([torch.randperm(w, generator=g), torch.randperm(w, generator=g)]).to(I32)
    ca, cb = torch.randn(2, w, generator=g), torch.randn(2, w, generator=g)
    cb[:, ::2] = 0.0
    t[..., 2], t[..., 3] = ca.view(I32), cb.view(I32)
    return t


def cases_gather(kind):
    lib = LIB
    n = len(GATHER_WIDTHS)
    for rows in (1, 5, 257):
        for form in ("index",) if kind == "plain" else ("index", "identity"):
            for table_aligned in (False, True) if kind == "sym" else (False,):
                def build(seed, rows=rows, form=form, table_aligned=table_aligned):
                    r, u, g = _rng(seed)
                    src_rows = rows if form == "identity" else GATHER_SRC_ROWS
                    images = 3 if kind == "sym" else 1
                    args = []
                    for k, w in enumerate(GATHER_WIDTHS):
                        args += [Arg(f"src{k}", "in", r(src_rows, w)), Arg(f"dst{k}", "out", shape=(images * rows, w))]
                    if form == "index":
                        args.append(Arg("idx", "in", _gather_idx(rows, g), in_fill=0))
                    normed = (0, 2) if kind != "plain" else ()
                    for k in normed:
                        args += [Arg(f"mean{k}", "in", r(GATHER_WIDTHS[k]) * 0.5), Arg(f"inv{k}", "in", u(GATHER_WIDTHS[k]) + 0.5)]
                    tabled = (0, 1) if kind == "sym" else ()
                    for k in tabled:
                        args.append(Arg(f"table{k}", "in", _sym_table(GATHER_WIDTHS[k], g), place="aligned" if table_aligned else None))

                    def call(t):
                        src, dst = _vp([t[f"src{k}"] for k in range(n)]), _vp([t[f"dst{k}"] for k in range(n)])
                        if kind == "plain":
                            return lib.tfp_gather_rows(src, dst, _ip(GATHER_WIDTHS), n, _p(t["idx"]), rows, _stream())
                        mean, inv = _vp([t.get(f"mean{k}") for k in range(n)]), _vp([t.get(f"inv{k}") for k in range(n)])
                        clip = (C.c_float * n)(*[5.0 if k in normed else 0.0 for k in range(n)])
                        if kind == "norm":
                            return lib.tfp_gather_rows_norm(src, dst, _ip(GATHER_WIDTHS), mean, inv, clip, n, _p(t.get("idx")), rows, _stream())
                        return lib.tfp_gather_rows_sym(src, dst, _ip(GATHER_WIDTHS), mean, inv, clip, _vp([t.get(f"table{k}") for k in range(n)]), n, _p(t.get("idx")),
                                                       rows, _stream())
                    refuse = {"offset": -1} if (kind == "sym" and not table_aligned) else None          # a symmetry table off 16 bytes
                    return Case(args, call, refuse=refuse, path={"offset": "refusal" if refuse else "the one instantiation"})
                yield f"rows{rows}-{form}{'-table_aligned' if table_aligned else ''}", build


# ---- the objective ---------------------------------------------------------------------------------------------------------------------------------------
def _loss_inputs(B, A, seed):
    from leibnizgym_amd.ppo import neglogp
    r, _, _ = _rng(seed)
    mu, ls, v = r(B, A) * 0.8, r(A) * 0.3 - 0.5, r(B)
    act, old_mu = mu + r(B, A) * 0.6, mu + r(B, A) * 0.05
    adv, ret = r(B), v + r(B) * 0.3
    old_nlp = neglogp(act, old_mu, ls.expand_as(old_mu)) + r(B) * 0.05
    w = (torch.rand(B, generator=torch.Generator().manual_seed(seed + 1)) < 0.8).float()
    return dict(mu=mu, log_std=ls, act=act, old_nlp=old_nlp, adv=adv, old_mu=old_mu, v=v, ret=ret, old_v=v + r(B) * 0.3, adv_w=torch.stack([adv, w], 1).contiguous())


LOSS_VARIANTS = {
    # entry point: (old_v, weighted, kl_rows of B or None, diag)
    "tfp_ppo_loss": (False, False, None, False), "tfp_ppo_loss_vclip": (True, False, None, False), "tfp_ppo_loss_w": (False, True, None, False),
    "tfp_ppo_loss_vclip_w": (True, True, None, False), "tfp_ppo_loss_sym": (True, True, lambda B: max(1, B // 3), False),
    "tfp_ppo_loss_diag": (True, True, lambda B: 0, True),
}


def cases_loss(entry):
    lib = LIB
    vclip, weighted, kl, diag = LOSS_VARIANTS[entry]
    coef = (0.2, 1.0, 0.003, 1e-4)
    for B in (1, 255, 257):
        for A in (9, 18):
            # adv_w off 8 bytes and a diag record off 8 bytes are refused (-1); with them kept aligned the rest of the arguments run offset
            modes = ["all"] + (["adv_w_aligned"] if weighted else []) + (["diag_off8"] if diag else [])
            for mode in modes:
                def build(seed, B=B, A=A, mode=mode):
                    d = _loss_inputs(B, A, seed)
                    keep = "aligned" if mode in ("adv_w_aligned", "diag_off8") else None
                    args = [Arg(k, "in", d[k]) for k in ("mu", "log_std", "act", "old_nlp", "old_mu", "v", "ret")]
                    args.append(Arg("adv_w", "in", d["adv_w"], place=keep) if weighted else Arg("adv", "in", d["adv"]))
                    if vclip:
                        args.append(Arg("old_v", "in", d["old_v"]))
                    args += [Arg("d_mu", "out", shape=(B, A)), Arg("d_v", "out", shape=(B,)), Arg("d_logstd", "out", shape=(A,), cmp=DLS_TOL),
                             Arg("loss", "out", shape=(1,), cmp=STATS_TOL), Arg("stats", "inout", torch.zeros(4), cmp=STATS_TOL)]
                    if diag:                                   # the record is int64 [16]; as int32 [32] its `offset` placement is 4 bytes past 16: off 8
                        rec = pk.new_diag("cpu")
                        args.append(Arg("diag", "inout", rec.view(I32) if mode == "diag_off8" else rec))

                    def call(t):
                        head = [_p(t[k]) for k in ("mu", "log_std", "act", "old_nlp")] + [_p(t["adv_w"] if weighted else t["adv"])] + [_p(t[k]) for k in ("old_mu", "v", "ret")]
                        tail = [B, A, *coef] + [_p(t[k]) for k in ("d_mu", "d_v", "d_logstd", "loss", "stats")] + [_stream()]
                        if entry in ("tfp_ppo_loss_sym", "tfp_ppo_loss_diag"):
                            return getattr(lib, entry)(*head, _p(t["old_v"]), 1, kl(B), *tail, *([_p(t["diag"])] if diag else []))
                        return getattr(lib, entry)(*head, *([_p(t["old_v"])] if vclip else []), *tail)
                    refuse = {"offset": -1} if ((weighted and mode == "all") or mode == "diag_off8") else None
                    return Case(args, call, refuse=refuse, path={"offset": "refusal" if refuse else "the one instantiation"})
                yield f"B{B}-A{A}-{mode}", build


# ---- the optimiser ---------------------------------------------------------------------------------------------------------------------------------------
ADAM_GROUPS = _flat_layout([(400, 41), (9, 100)])[1], _flat_layout([(400, 113), (1, 100)])[1]         # the buffers of test_flat_clip_adam_matches_torch


def _diag_cmp(got, want, what):
    """the optimiser's slots: STEPS and TRUNC exact; the norm slots (fixed-point sums, float bit patterns) follow `sq`, a float atomic sum over blocks: the
    relative bound tests/test_ppo_diagnostics_gpu.py holds them to against the norms themselves"""
    assert torch.equal(got[:12], want[:12]), f"{what}: counters {got[:12].tolist()} != {want[:12].tolist()}"
    for q in (12, 13):
        torch.testing.assert_close(got[q].double(), want[q].double(), rtol=DIAG_GN_REL, atol=0.0, msg=lambda m: f"{what}: slot {q}: {m}")
    for q in (14, 15):
        torch.testing.assert_close(got[q:q + 1].to(I32).view(F32), want[q:q + 1].to(I32).view(F32), rtol=DIAG_GN_REL, atol=0.0, msg=lambda m: f"{what}: slot {q}: {m}")


def cases_clip_adam(diag):
    lib = LIB
    n0_, n1_ = ADAM_GROUPS
    assert n0_ % 4 == 0 and n1_ % 4 == 0
    for groups, (n0, n1) in (("two_groups", (n0_, n0_ + n1_)), ("one_group", (n0_, n0_))):
        for truncating in (False, True):
            def build(seed, n0=n0, n1=n1, truncating=truncating):
                r, u, _ = _rng(seed)
                # without truncation the coefficient is exactly 1 and parameters and moments do not depend on the order `sq` was summed in: bits.  With it they
                # follow the float atomics of the squared norms: the tolerance of the optimiser's own test
                c = ADAM_TOL if truncating else "bits"
                step0 = torch.tensor([3.0, 3.0])
                sq0 = torch.zeros(4)
                args = [Arg("p", "inout", r(n1) * 0.1, cmp=c), Arg("g", "in", r(n1) * (10.0 if truncating else 1e-3)), Arg("m", "inout", r(n1) * 0.01, cmp=c),
                        Arg("v", "inout", u(n1) * 1e-4, cmp=c), Arg("sq", "inout", sq0, cmp=SQ_TOL), Arg("step", "inout", step0),
                        Arg("lr", "in", torch.tensor([3e-4, 5e-4]))]
                if diag:
                    args.append(Arg("diag", "inout", pk.new_diag("cpu"), cmp=_diag_cmp))

                def call(t):
                    a = [_p(t[k]) for k in ("p", "g", "m", "v")] + [n0, n1] + [_p(t[k]) for k in ("sq", "step", "lr")] + [1.0, 0.5, 0.9, 0.999, 1e-8, _stream()]
                    return lib.tfp_clip_adam_diag(*a, _p(t["diag"])) if diag else lib.tfp_clip_adam(*a)
                return Case(args, call, path={"offset": "the one instantiation"})
            yield f"{groups}-{'truncating' if truncating else 'untruncated'}", build
    if diag:
        def build_off8(seed):
            r, u, _ = _rng(seed)
            n = n0_
            args = [Arg("p", "inout", r(n)), Arg("g", "in", r(n)), Arg("m", "inout", r(n)), Arg("v", "inout", u(n)), Arg("sq", "inout", torch.zeros(4), cmp=SQ_TOL),
                    Arg("step", "inout", torch.zeros(2)), Arg("lr", "in", torch.tensor([3e-4, 5e-4])), Arg("diag", "inout", pk.new_diag("cpu").view(I32), cmp=None)]
            call = lambda t: lib.tfp_clip_adam_diag(*[_p(t[k]) for k in ("p", "g", "m", "v")], n, n, *[_p(t[k]) for k in ("sq", "step", "lr")], 1e3, 1e3,      # noqa: E731
                                                    0.9, 0.999, 1e-8, _stream(), _p(t["diag"]))
            return Case(args, call, refuse={"offset": -1}, path={"offset": "refusal"})
        yield "diag_off8", build_off8


# ---- rollout bookkeeping --------------------------------------------------------------------------------------------------------------------------------
BOOK_N, BOOK_T = (1, 63, 65, 257), (1, 3)


def _env_buffers(n, seed, prefix=""):
    """what the bookkeeping kernels read of an engine: a state of finite rows with unit quaternions, reward, flags and step counters in which episodes
    begin (steps == 1), run, end (reset_buf) and time out (steps >= 4)"""
    r, u, g = _rng(seed)
    state = r(capi.TF_STATE_ROWS, n) * 0.1
    for q0 in (capi.S_CUBE_Q, capi.S_GOAL_Q):
        q = r(4, n)
        state[q0:q0 + 4] = q / q.norm(dim=0, keepdim=True)
    return [Arg(prefix + "state", "in", state), Arg(prefix + "reward", "in", r(n)), Arg(prefix + "reset_buf", "in", u(n) < 0.4),
            Arg(prefix + "goal_reset_buf", "in", u(n) < 0.3), Arg(prefix + "steps", "in", torch.randint(1, 6, (n,), generator=g, dtype=I64), in_fill=0)]


def cases_rollout_record():
    lib = LIB
    for n in BOOK_N:
        for Ds in (113, 0):
            def build(seed, n=n, Ds=Ds):
                r, _, _ = _rng(seed)
                Do, A = 41, 9
                ls = 0.3 * r(A)
                args = [Arg("obs", "in", r(n, Do)), Arg("mu", "in", r(n, A)), Arg("log_std", "in", ls), Arg("sigma", "in", ls.exp()), Arg("eps", "in", r(n, A)),
                        Arg("val", "in", r(n))]
                args += [Arg(k, "out", shape=s) for k, s in (("b_obs", (n, Do)), ("b_act", (n, A)), ("b_mu", (n, A)), ("b_nlp", (n,)), ("b_val", (n,)))]
                if Ds:
                    args += [Arg("states", "in", r(n, Ds)), Arg("b_states", "out", shape=(n, Ds))]
                return Case(args, lambda t: lib.tfp_rollout_record(_p(t["obs"]), Do, _p(t.get("states")), Ds, _p(t["mu"]), _p(t["log_std"]), _p(t["sigma"]), _p(t["eps"]),
                                                                   _p(t["val"]), n, A, _p(t["b_obs"]), _p(t.get("b_states")), _p(t["b_act"]), _p(t["b_mu"]),
                                                                   _p(t["b_nlp"]), _p(t["b_val"]), _stream()), path={"offset": "the one instantiation"})
            yield f"n{n}-Ds{Ds}", build


def cases_rollout_reward():
    lib = LIB
    for n in BOOK_N:
        def build(seed, n=n):
            r, u, _ = _rng(seed)
            args = [Arg("r", "in", r(n)), Arg("done", "in", u(n) < 0.3), Arg("b_rew", "out", shape=(n,)), Arg("b_done", "out", shape=(n,))]
            return Case(args, lambda t: lib.tfp_rollout_reward(_p(t["r"]), _p(t["done"]), 0.01, n, _p(t["b_rew"]), _p(t["b_done"]), _stream()))
        yield f"n{n}", build


def cases_rollout_flags():
    lib = LIB
    for n in BOOK_N:
        def build(seed, n=n):
            env = {a.name: a for a in _env_buffers(n, seed)}
            args = [env["reward"], env["reset_buf"], env["steps"]] + [Arg(k, "out", shape=(n,)) for k in ("b_rew", "b_end", "b_tout")]
            return Case(args, lambda t: lib.tfp_rollout_flags(_p(t["reward"]), _p(t["reset_buf"]), _p(t["steps"]), 0.01, 4, n, _p(t["b_rew"]), _p(t["b_end"]),
                                                              _p(t["b_tout"]), _stream()))
        yield f"n{n}", build


def cases_gae(entry):
    lib = LIB
    for n in BOOK_N:
        for T in BOOK_T:
            for vnorm in {"tfp_gae": (False,), "tfp_gae_vnorm": (True,), "tfp_gae_ends": (False, True)}[entry]:
                def build(seed, n=n, T=T, vnorm=vnorm):
                    r, u, _ = _rng(seed)
                    args = [Arg("rew", "in", r(T, n)), Arg("end", "in", (u(T, n) < 0.2).float()), Arg("val", "in", r(T + 1, n)), Arg("adv", "out", shape=(T, n)),
                            Arg("ret", "out", shape=(T, n))]
                    if vnorm:
                        args += [Arg("mean_f", "in", r(1)), Arg("inv_std_f", "in", u(1) + 0.5), Arg("ret_n", "out", shape=(T, n)), Arg("v_old_n", "out", shape=(T, n))]
                    if entry == "tfp_gae_ends":
                        args += [Arg("tout", "in", (u(T, n) < 0.3).float()), Arg("last_end", "in", (u(n) < 0.3).float()), Arg("w", "out", shape=(T, n))]
                    g, gt, clip = 0.99, 0.99 * 0.95, 5.0

                    def call(t):
                        if entry == "tfp_gae":
                            return lib.tfp_gae(_p(t["rew"]), _p(t["end"]), _p(t["val"]), g, gt, T, n, _p(t["adv"]), _p(t["ret"]), _stream())
                        if entry == "tfp_gae_vnorm":
                            return lib.tfp_gae_vnorm(_p(t["rew"]), _p(t["end"]), _p(t["val"]), _p(t["mean_f"]), _p(t["inv_std_f"]), clip, g, gt, T, n, _p(t["adv"]),
                                                     _p(t["ret"]), _p(t["ret_n"]), _p(t["v_old_n"]), _stream())
                        return lib.tfp_gae_ends(_p(t["rew"]), _p(t["end"]), _p(t["tout"]), _p(t["val"]), _p(t["last_end"]), 1, _p(t.get("mean_f")),
                                                _p(t.get("inv_std_f")), clip if vnorm else 0.0, g, gt, T, n, _p(t["adv"]), _p(t["ret"]), _p(t["w"]), _p(t.get("ret_n")),
                                                _p(t.get("v_old_n")), _stream())
                    return Case(args, call)
                yield f"n{n}-T{T}{'-vnorm' if vnorm and entry == 'tfp_gae_ends' else ''}", build


def cases_rollout_track():
    lib = LIB
    for n in BOOK_N:
        for mode in ("A", "B"):
            def build(seed, n=n, mode=mode):
                r, u, g = _rng(seed + 7)
                env = {a.name: a for a in _env_buffers(n, seed)}
                trk = torch.stack([r(n).view(I32), (u(n) < 0.6).to(I32)])                      # running returns, and most envs armed: their episodes count
                args = [env[k] for k in ("state", "reward", "reset_buf", "steps")] + [Arg("env_trk", "inout", trk), Arg("acc", "inout", torch.zeros(pk.TRACK_ACC, dtype=I64)),
                                                                                       Arg("b_rew", "out", shape=(n,))]
                args += [Arg("done", "in", u(n) < 0.3), Arg("b_done", "out", shape=(n,))] if mode == "A" else [Arg("b_end", "out", shape=(n,)), Arg("b_tout", "out", shape=(n,))]

                def call(t):
                    a = pk.TfpTrackArgs()
                    for k in ("state", "reward", "reset_buf", "steps", "b_rew", "b_done", "b_end", "b_tout", "env_trk", "acc"):
                        setattr(a, k, _p(t.get(k)))
                    a.done_bytes = _p(t.get("done"))
                    a.episode_length, a.scale, a.pos_tol, a.ori_tol, a.rule, a.N = 4, 0.01, 0.2, 2.0, 1, n
                    return lib.tfp_rollout_track(C.byref(a), _stream())
                return Case(args, call)
            yield f"n{n}-mode{mode}", build


def cases_record_step():
    lib = LIB
    for n in BOOK_N:
        def build(seed, n=n):
            r, u, g = _rng(seed + 7)
            env = {a.name: a for a in _env_buffers(n, seed)}
            W, L = max(1, n - 1), 3                                                              # the last env is not watched
            rec = torch.zeros(pk.REC_ENV_ROWS, W, dtype=I32)
            rec[0] = torch.randint(0, 3, (W,), generator=g).to(I32)                              # idle, armed, frozen
            rec[1] = torch.randint(0, 5, (W,), generator=g).to(I32)
            rec[4] = r(W).view(I32)
            args = [env[k] for k in ("state", "reward", "reset_buf", "steps")]
            args += [Arg("ring", "inout", r(L, pk.REC_ROWS, W)), Arg("hdr", "inout", r(capi.TF_NUM_DR, W)), Arg("env_rec", "inout", rec),
                     Arg("acc", "inout", torch.zeros(pk.REC_ACC, dtype=I64))]

            def call(t):
                a = pk.TfpRecordArgs()
                for k in ("state", "reward", "reset_buf", "steps", "ring", "hdr", "env_rec", "acc"):
                    setattr(a, k, _p(t[k]))
                a.episode_length, a.pos_tol, a.ori_tol, a.N, a.W, a.L, a.every, a.select, a.rule = 4, 0.2, 2.0, n, W, L, 2, 7, 1
                return lib.tfp_record_step(C.byref(a), _stream())
            return Case(args, call)
        yield f"n{n}", build


def cases_eval_step():
    lib = LIB
    for n in BOOK_N:
        def build(seed, n=n):
            r, u, g = _rng(seed + 7)
            env = _env_buffers(n, seed)
            acc_env = torch.stack([r(n).view(I32), torch.randint(0, 3, (n,), generator=g).to(I32), torch.randint(0, 3, (n,), generator=g).to(I32),
                                   torch.randint(0, 3, (n,), generator=g).to(I32)])
            args = env + [Arg("env_acc", "inout", acc_env), Arg("acc", "inout", torch.zeros(evaluate.ACC, dtype=I64))]
            return Case(args, lambda t: lib.tfp_eval_step(_p(t["state"]), _p(t["reward"]), _p(t["reset_buf"]), _p(t["goal_reset_buf"]), _p(t["steps"]), _p(t["env_acc"]),
                                                          _p(t["acc"]), n, 0.2, 2.0, 1, 2, _stream()))
        yield f"n{n}", build


def cases_eval_test_predicates():
    lib = LIB
    for n in BOOK_N:
        def build(seed, n=n):
            env = {a.name: a for a in _env_buffers(n, seed)}
            args = [env["state"], Arg("out", "inout", torch.zeros(2, dtype=I64))]
            return Case(args, lambda t: lib.tfp_eval_test_predicates(_p(t["state"]), n, 0.2, 2.0, _p(t["out"]), _stream()))
        yield f"n{n}", build


# ---- running moments ------------------------------------------------------------------------------------------------------------------------------------
def cases_moments():
    lib = LIB
    for rows in (1, 63, 1025):
        for D in ([1], [41], [113], [113, 41]):                              # k = 1 and k = 2 arrays over the same rows
            def build(seed, rows=rows, D=D):
                r, _, _ = _rng(seed)
                need = int(lib.tfp_moments_part_doubles(_ip(D), len(D), rows))
                args = [Arg(f"x{k}", "in", r(rows, d) * 2.0 + 0.5) for k, d in enumerate(D)]
                args += [Arg("part", "out", shape=(max(need, 1),), dtype=F64, full=False), Arg("out", "out", shape=(sum(1 + 2 * d for d in D),), dtype=F64)]
                return Case(args, lambda t: lib.tfp_moments(_vp([t[f"x{k}"] for k in range(len(D))]), _ip(D), len(D), rows, _p(t["part"]), need, _p(t["out"]), _stream()))
            yield f"rows{rows}-D{'_'.join(map(str, D))}", build


def cases_norm_merge():
    lib = LIB
    for D in ([1], [41], [113, 41]):
        for k in (1, 2):
            def build(seed, D=D, k=k):
                r, u, _ = _rng(seed)
                rec = lambda d, cnt: torch.cat([torch.tensor([float(cnt)]), r(d), u(d) * cnt]).double()                 # noqa: E731  {count, mean, M2}
                stride = sum(1 + 2 * d for d in D) + 3                                      # the records of a rank, and a gap
                args = []
                for q, d in enumerate(D):
                    batch = torch.zeros((k - 1) * stride + 1 + 2 * d, dtype=F64)
                    for j in range(k):
                        batch[j * stride:j * stride + 1 + 2 * d] = rec(d, 63 + j)
                    args += [Arg(f"run{q}", "inout", rec(d, 1000)), Arg(f"batch{q}", "in", batch), Arg(f"mean_f{q}", "out", shape=(d,)), Arg(f"inv_std_f{q}", "out", shape=(d,))]
                n = len(D)
                ls = lambda t, name: _vp([t[f"{name}{q}"] for q in range(n)])                                              # noqa: E731
                return Case(args, lambda t: lib.tfp_norm_merge(ls(t, "run"), ls(t, "batch"), _ip(D), n, k, stride, ls(t, "mean_f"), ls(t, "inv_std_f"), _stream()))
            yield f"D{'_'.join(map(str, D))}-k{k}", build


# ---- the renderer and the leaf kernels of the golden-vector tests ------------------------------------------------------------------------------------------
RENDER_N, RENDER_SIZE, RENDER_VIEWS = 16, 64, [0, 5, 9]          # the smallest env count and image of tests/test_render_gpu.py


def _reset_state(n, seed=3):
    """the state rows of a freshly reset engine (host copy)"""
    from leibnizgym_amd.engine import TrifingerEngine, make_config
    hip = capi.load_hip_library()
    eng = TrifingerEngine(make_config(hip, n, seed=seed, **pu.CONFIGS["d4_torque_asym"]), device=DEV, lib=hip)
    eng.reset()
    state = eng.state.detach().cpu().clone()
    eng.close()
    return state


def cases_render(entry):
    from leibnizgym_amd import render as rd

    def build(seed):
        r, _, _ = _rng(seed)
        rr = rd.SceneRenderer(None, width=RENDER_SIZE, height=RENDER_SIZE, max_views=len(RENDER_VIEWS), device=DEV)
        rr.set_views(RENDER_VIEWS, RENDER_N)
        V, H = len(RENDER_VIEWS), RENDER_SIZE
        args = [Arg("state", "in", _reset_state(RENDER_N))]
        if entry == "tfr_render":               # a colour byte may be 0xA5 by right: `full` cannot be asked of it - the alpha channel is, below
            args += [Arg("color", "out", shape=(V, H, H, 4), dtype=U8, full=False), Arg("depth", "out", shape=(V, H, H)), Arg("segmentation", "out", shape=(V, H, H), dtype=U8)]
            call = lambda t: rr.lib.tfr_render(rr._handle, _p(t["state"]), _p(t["color"]), _p(t["depth"]), _p(t["segmentation"]), _stream())      # noqa: E731

            def after(t, handles):
                assert bool((t["color"][..., 3] == 255).all()), "a pixel was not written (alpha is 255 everywhere)"
                assert int(t["segmentation"].max()) < rd.NUM_IDS and len(torch.unique(t["segmentation"])) >= 5
        else:
            n = 257
            pts = r(n, 3) * torch.tensor([0.15, 0.15, 0.1]) + torch.tensor([0.0, 0.0, 0.1])
            args += [Arg("points", "in", pts), Arg("dist", "out", shape=(n,)), Arg("id", "out", shape=(n,), dtype=U8), Arg("boundary_dist", "out", shape=(n,))]
            call = lambda t: rr.lib.tfr_test_field(rr._handle, _p(t["state"]), 5, _p(t["points"]), _p(t["dist"]), _p(t["id"]), _p(t["boundary_dist"]), n, _stream())   # noqa: E731
            after = None
        case = Case(args, call, after=after, path={"offset": "the one instantiation"})
        case.keep = rr                                                               # the handle lives as long as the case
        return case
    yield f"{RENDER_SIZE}x{RENDER_SIZE}-{RENDER_N}envs", build


def cases_leaf(entry):
    hip_lib = lambda: capi.load_hip_library()                                                                               # noqa: E731
    n = 65

    def build(seed):
        r, u, g = _rng(seed)
        hip = hip_lib()
        quat = lambda: (lambda q: q / q.norm(dim=1, keepdim=True))(r(n, 4))                                                  # noqa: E731
        keep = None
        if entry in ("tf_test_quat_diff_rad", "tf_test_quat_mul"):
            args = [Arg("a", "in", quat()), Arg("b", "in", quat()), Arg("out", "out", shape=(n,) if entry.endswith("rad") else (n, 4))]
            call = lambda t: getattr(hip, entry)(_p(t["a"]), _p(t["b"]), _p(t["out"]), n, _stream())                        # noqa: E731
        elif entry == "tf_test_lgsk":
            args = [Arg("x", "in", r(n)), Arg("out", "out", shape=(n,))]
            call = lambda t: hip.tf_test_lgsk(_p(t["x"]), 30.0, _p(t["out"]), n, _stream())                                 # noqa: E731
        elif entry == "tf_test_sample_xy":
            args = [Arg("u_radius", "in", u(n)), Arg("u_theta", "in", u(n)), Arg("x", "out", shape=(n,)), Arg("y", "out", shape=(n,))]
            call = lambda t: hip.tf_test_sample_xy(_p(t["u_radius"]), _p(t["u_theta"]), 0.1, _p(t["x"]), _p(t["y"]), n, _stream())    # noqa: E731
        elif entry in ("tf_test_sample_yaw_quat", "tf_test_normalize_quat"):
            args = [Arg("u", "in", u(n) if entry.endswith("yaw_quat") else r(n, 4)), Arg("quat", "out", shape=(n, 4))]
            call = lambda t: getattr(hip, entry)(_p(t["u"]), _p(t["quat"]), n, _stream())                                   # noqa: E731
        elif entry == "tf_test_philox":
            args = [Arg("env_id", "in", torch.randint(0, 2 ** 20, (n,), generator=g).to(I32)), Arg("counter", "in", torch.randint(0, 99, (n,), generator=g).to(I32)),
                    Arg("out4", "out", shape=(n, 4), dtype=I32, full=False)]               # any 32-bit pattern is a legitimate draw
            call = lambda t: hip.tf_test_philox(0x1234567890ABCDEF, _p(t["env_id"]), _p(t["counter"]), 3, _p(t["out4"]), n, _stream())   # noqa: E731
        else:
            from leibnizgym_amd.engine import TrifingerEngine, make_config
            keep = TrifingerEngine(make_config(hip, 1), device=DEV, lib=hip)
            args = [Arg("q", "in", r(n, 3) * 0.5), Arg("qd", "in", r(n, 3)), Arg("tip", "out", shape=(n, 3)), Arg("mass", "out", shape=(n, 9)), Arg("bias", "out", shape=(n, 3))]
            call = lambda t: hip.tf_test_finger_dynamics(keep._handle, _p(t["q"]), _p(t["qd"]), _p(t["tip"]), _p(t["mass"]), _p(t["bias"]), n, _stream())   # noqa: E731
        case = Case(args, call, path={"offset": "the one instantiation"})
        case.keep = keep
        return case
    yield f"n{n}", build


# ---- THE TABLE: (entry points the row covers, case generator) ---------------------------------------------------------------------------------------------
TABLE = [
    (("tfp_linear_fwd",), cases_linear_fwd), (("tfp_gemm_nn",), cases_gemm_nn), (("tfp_gemm_nn_dz",), cases_gemm_nn_dz), (("tfp_gemm_tn_bias",), cases_gemm_tn_bias),
    (("tfp_gemm_tn_partials", "tfp_sum_partials_multi"), cases_gemm_tn_partials), (("tfp_linear_fwd_group",), cases_linear_fwd_group),
    (("tfp_gemm_nn_group",), lambda: cases_gemm_nn_group(False)), (("tfp_gemm_nn_dz_group",), lambda: cases_gemm_nn_group(True)),
    (("tfp_gemm_tn_partials_group",), cases_gemm_tn_partials_group),
    (("tfp_gemm_tn_partials_direct",), lambda: cases_gemm_tn_partials_direct(False)), (("tfp_gemm_tn_partials_direct_bf16",), lambda: cases_gemm_tn_partials_direct(True)),
    (("tfp_mlp_forward",), lambda: cases_walk("plain", "forward")), (("tfp_mlp_backward",), lambda: cases_walk("plain", "backward")),
    (("tfp_mlp_forward_norm",), lambda: cases_walk("stats", "forward")),
    (("tfp_mlp_forward_norm",), lambda: cases_walk("stats", "forward", NORM_WALK_SHAPES, stats_for=(0, 1))),
    (("tfp_net_forward",), lambda: cases_walk("ext", "forward")), (("tfp_net_backward",), lambda: cases_walk("ext", "backward")),
    (("tfp_net_forward_bf16",), lambda: cases_walk("bf16", "forward")), (("tfp_net_backward_bf16",), lambda: cases_walk("bf16", "backward")),
    (("tfp_gather_rows",), lambda: cases_gather("plain")), (("tfp_gather_rows_norm",), lambda: cases_gather("norm")), (("tfp_gather_rows_sym",), lambda: cases_gather("sym")),
] + [((e,), (lambda e=e: cases_loss(e))) for e in LOSS_VARIANTS] + [
    (("tfp_clip_adam",), lambda: cases_clip_adam(False)), (("tfp_clip_adam_diag",), lambda: cases_clip_adam(True)),
    (("tfp_rollout_record",), cases_rollout_record), (("tfp_rollout_reward",), cases_rollout_reward), (("tfp_rollout_flags",), cases_rollout_flags),
] + [((e,), (lambda e=e: cases_gae(e))) for e in ("tfp_gae", "tfp_gae_vnorm", "tfp_gae_ends")] + [
    (("tfp_rollout_track",), cases_rollout_track), (("tfp_record_step",), cases_record_step), (("tfp_eval_step",), cases_eval_step),
    (("tfp_eval_test_predicates",), cases_eval_test_predicates), (("tfp_moments",), cases_moments), (("tfp_norm_merge",), cases_norm_merge),
    (("tfr_render",), lambda: cases_render("tfr_render")), (("tfr_test_field",), lambda: cases_render("tfr_test_field")),
] + [((e,), (lambda e=e: cases_leaf(e))) for e in ("tf_test_quat_diff_rad", "tf_test_quat_mul", "tf_test_lgsk", "tf_test_sample_xy", "tf_test_sample_yaw_quat",
                                                    "tf_test_normalize_quat", "tf_test_philox", "tf_test_finger_dynamics")]


def covered_entry_points():
    return sorted({name for names, _ in TABLE for name in names} | set(STEP_ENTRY_POINTS))


def _all_cases():
    out = []
    for names, gen in TABLE:
        for k, (ident, build) in enumerate(gen()):
            out.append(pytest.param(build, 1000 * len(out) + 17, id=f"{names[0]}-{ident}"))
    return out


# ---- running a case --------------------------------------------------------------------------------------------------------------------------------------
def _materialise(case, placement):
    """-> (name -> tensor on the GPU, handles).  placement None: plain exact-sized tensors; an output then starts from the sentinel too, so that what a call
    is documented to leave unwritten compares equal"""
    t, handles = {}, []
    for a in case.args:
        if placement is None:
            if a.role == "out":
                x = gu.sentinel_filled(a.shape, a.dtype, DEV)
            else:
                x = a.data.to(DEV).clone()
            t[a.name] = x
            continue
        data = None if a.role == "out" else a.data.to(DEV)
        view, h = gu.banded(a.shape, a.dtype, DEV, a.role, a.place or placement, name=a.name, data=data, in_fill=a.in_fill, full=a.full, finite=a.finite)
        t[a.name] = view
        handles.append(h)
    return t, handles


def _compare(case, a, got, want, placement):
    how = a.alt if (placement in case.loose and a.alt is not None) else a.cmp
    what = f"`{a.name}` [{placement}]"
    if how is None:
        return
    if how == "bits":
        gu.assert_same_bits(got, want, what)
    elif callable(how):
        how(got, want, what)
    else:
        torch.testing.assert_close(got, want, rtol=how[0], atol=how[1], msg=lambda m: f"{what}: {m}")


@pytest.mark.gpu
@pytest.mark.parametrize("build,seed", _all_cases())
def test_entry_point_on_banded_buffers(hip, build, seed):
    case = build(seed)
    plain, _ = _materialise(case, None)
    assert case.call(plain) == 0, "the plain run is refused"
    torch.cuda.synchronize()
    for placement in gu.PLACEMENTS:
        t, handles = _materialise(case, placement)
        initial = {h.name: h.raw.clone() for h in handles if h.role != "in"}
        rc = case.call(t)
        torch.cuda.synchronize()
        if placement in case.refuse:                   # a documented refusal: the status, and nothing launched - every array as it was, the bands intact
            assert rc == case.refuse[placement], f"[{placement}] status {rc}, the header documents {case.refuse[placement]}"
            for h in handles:
                assert h.role == "in" or torch.equal(h.raw, initial[h.name]), f"[{placement}] refused, yet `{h.name}` was written"
            gu.check([_unfull(h) for h in handles])
            continue
        assert rc == 0, f"[{placement}] status {rc}"
        gu.check(handles)
        for a in case.args:
            if a.role != "in":
                _compare(case, a, t[a.name], plain[a.name], placement)
        if case.after is not None:
            case.after(t, handles)
    if case.after is not None:
        case.after(plain, [])


def _unfull(h):
    h.full = h.finite = False
    return h


# ---- the env step through re-bound buffers ----------------------------------------------------------------------------------------------------------------
STEP_N = (1, 65, 130)
# one cell per family of parity_util.MATRIX_FAMILIES: (A, ASYM) walk the four combinations in turn
STEP_FAMILIES = [(f, (9, 18)[i % 2], bool((i // 2) % 2)) for i, f in enumerate(pu.MATRIX_FAMILIES)]
STEP_CELLS = [pytest.param(f, a, asym, v, n, id=f"{'d' if f == (1, 1, 0) else ''}{pu.MATRIX_FAMILIES[f]}-A{a}-{'asym' if asym else 'sym'}-{v}-n{n}")
              for f, a, asym in STEP_FAMILIES for v in pu.VARIANTS if not (f[1] and v == "narrow") for n in STEP_N]          # the surface families have no `narrow`


def _matrix_rollout(hip, family, a, asym, variant, n, path, placement):
    eng = pu.matrix_engine(hip, DEV, family, a, asym, variant=variant, n=n, episode_length=gu.ROLLOUT_EPISODE)
    place = None
    if family[2] != 2 and n > pu.MATRIX_PLACE_FIRST:                 # the cubes of envs 65.. at the boundary, where the matrix places them
        place = lambda e: pu.place_cubes_at_the_boundary(e, e.cfg.model, first=pu.MATRIX_PLACE_FIRST)       # noqa: E731
    return gu.engine_rollout(eng, path, placement, seed=pu.MATRIX_SEED, place=place, round_trip=path == "step")


@pytest.mark.gpu
@pytest.mark.parametrize("family,a,asym,variant,n", STEP_CELLS)
def test_env_step_through_banded_buffers(hip, family, a, asym, variant, n):
    """tf_reset, then 12 steps in episodes of 4 - tf_step (and a load_state_dict round trip), tf_step_random, the five split-path entries - with every
    buffer of the engine a banded view and every action a banded input: the bands intact after every call, the action unchanged, every per-env field
    the bits of the same engine on its own buffers, `info` under assert_bit_equal's rule"""
    for path in gu.ROLLOUT_PATHS:
        want = _matrix_rollout(hip, family, a, asym, variant, n, path, None)
        steps = torch.tensor([s["steps"].tolist() for s in want[:1 + gu.ROLLOUT_STEPS]])
        assert int((steps[1:] < steps[:-1]).sum()) >= 2 * n, "no time-outs inside the run"
        for placement in gu.PLACEMENTS:
            got = _matrix_rollout(hip, family, a, asym, variant, n, path, placement)
            assert len(got) == len(want)
            for t, (x, y) in enumerate(zip(got, want)):
                pu.assert_bit_equal(x, y, f"{family} [{variant}] n={n} {path} [{placement}] snapshot {t}")
