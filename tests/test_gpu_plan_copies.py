"""GPU: sf_plan_copies_device against the dict model (tests/plan_expect.py).

The C-ABI is called directly, with every output among 0xEE bytes of its own
tensor, so "nothing written" is checked byte for byte; hashlib stands for the
explicit-list kernel in the model.  Block counts around the wave and the
workgroup (63 .. 257) and a few thousand; candidate counts around 65, where the
explicit-list launch starts sorting by length class; one local file read by 300
jobs (one counter under 300 atomics); the read-backs and the candidates hashed
through sf_test_plan_copies_stats; the call behind a hold on a fresh stream
(tests/stream_order.py); and the job lists carried out by
sf_copy_blocks_device."""
import ctypes

import numpy as np
import pytest
import torch

import plan_expect as pe
import stream_order as so
from syncfast_amd import _lib, device

pytestmark = pytest.mark.gpu

FILL = 0xEE
EXTRA = 3  # entries every output has beyond what the call may write
INPUTS = (("digests", np.uint8), ("sizes", np.uint32), ("offsets", np.uint64), ("rows", np.int64),
          ("block_file", np.uint32), ("file_base", np.uint64), ("table_file", np.uint32), ("table_offset", np.uint64),
          ("table_size", np.uint32), ("local_base", np.uint64), ("local_size", np.uint64), ("src", np.uint8))
SIGNED = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}


def host_arrays(case) -> dict:
    """The case's lists as the numpy arrays the device gets (unsigned values in
    the signed dtypes torch has)."""
    out = {}
    for name, dtype in INPUTS:
        v = case[name]
        a = np.frombuffer(b"".join(v) if name == "digests" else v, np.uint8) if name in ("digests", "src") \
            else np.array(v, dtype)
        a = a.reshape(-1, 20) if name == "digests" else a
        out[name] = a.view(SIGNED.get(a.dtype, a.dtype)).copy()
    return out


def on_device(case, gpu) -> dict:
    return {k: torch.from_numpy(v).to(gpu) for k, v in host_arrays(case).items()}


def outputs(n, n_local, cap, gpu) -> dict:
    """Every output of a call, EXTRA entries longer than it may be written, full of FILL."""
    shapes = {"present": (n, 1), "ask": (n, 1), "dst": (n, 8), "src_offsets": (cap, 8), "dst_offsets": (cap, 8),
              "job_sizes": (cap, 4), "job_blocks": (cap, 8), "local_jobs": (n_local, 4)}
    return {k: torch.full(((rows + EXTRA) * width,), FILL, dtype=torch.uint8, device=gpu)
            for k, (rows, width) in shapes.items()}


def call(x, o, n, cap, gpu, query=False, verify=True, drop=()):
    """The C call over device inputs x and outputs o; `drop`: outputs passed as
    NULL.  Returns (rc, counts)."""
    p = lambda t: t.data_ptr() if t is not None and t.numel() else None  # noqa: E731
    q = {k: (None if k in drop else v.data_ptr()) for k, v in o.items()}
    counts = (ctypes.c_uint64 * 8)(*[77] * 8)
    src = x["src"] if verify else None
    rc = _lib.lib().sf_plan_copies_device(
        p(x["digests"]), p(x["sizes"]), p(x["offsets"]), p(x["rows"]), p(x["block_file"]), n,
        p(x["file_base"]), x["file_base"].numel(), p(x["table_file"]), p(x["table_offset"]), p(x["table_size"]),
        x["table_file"].numel(), None if query else x["local_base"].data_ptr(), p(x["local_size"]),
        x["local_size"].numel(), p(src), x["src"].numel(), q["present"], q["ask"], q["dst"], q["src_offsets"],
        q["dst_offsets"], q["job_sizes"], q["job_blocks"], cap, q["local_jobs"], counts,
        torch.cuda.current_stream(gpu).cuda_stream)
    return rc, list(counts)


def expected_bytes(m, n, n_local, cap, lists=True) -> dict:
    """What every output holds after a call the model answered with m: the
    written rows, and FILL in the rest.  lists False: d_local_jobs alone."""
    def fill(rows, width, values, dtype):
        a = np.full((rows + EXTRA) * width, FILL, np.uint8)
        b = np.array(values, dtype).view(np.uint8)
        a[:b.size] = b
        return a
    jobs = m["jobs"] if lists else []
    col = lambda k: [j[k] for j in jobs]  # noqa: E731
    none = []
    return {"present": fill(n, 1, m["present"] if lists else none, np.uint8),
            "ask": fill(n, 1, m["ask"] if lists else none, np.uint8),
            "dst": fill(n, 8, m["dst"] if lists else none, np.uint64),
            "src_offsets": fill(cap, 8, col(0), np.uint64), "dst_offsets": fill(cap, 8, col(1), np.uint64),
            "job_sizes": fill(cap, 4, col(2), np.uint32), "job_blocks": fill(cap, 8, col(3), np.int64),
            "local_jobs": fill(n_local, 4, m["local_jobs"], np.uint32)}


def check_outputs(o, want):
    torch.cuda.synchronize()
    for k, t in o.items():
        got = t.cpu().numpy()
        bad = np.flatnonzero(got != want[k])
        assert bad.size == 0, f"{k}: bytes {bad[:8].tolist()} are {got[bad[:8]].tolist()}, want {want[k][bad[:8]].tolist()}"


def model_of(case, query=False, verify=True):
    return pe.plan_model(**dict(case, local_base=None if query else case["local_base"],
                                src=case["src"] if verify else None))


def stats():
    out = (ctypes.c_uint64 * 4)()
    assert _lib.lib().sf_test_plan_copies_stats(out) == 0
    return list(out)


@pytest.mark.parametrize("verify", [True, False], ids=["verified", "trusted"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 3000])
def test_plan_is_the_models(gpu, n, verify):
    case = pe.mixed_case(n, n)
    m = model_of(case, verify=verify)
    if n >= 63:  # every class at once
        assert all(c > 0 for k, c in zip(pe.COUNTS, m["counts"]) if k != "unverified" or verify)
    x, nl = on_device(case, gpu), len(case["local_size"])
    cap = len(m["jobs"])  # exactly enough
    o = outputs(n, nl, cap, gpu)
    rc, counts = call(x, o, n, cap, gpu, verify=verify)
    assert (rc, counts) == (0, m["counts"])
    check_outputs(o, expected_bytes(m, n, nl, cap))
    hashed = m["candidates"]
    assert stats() == [2 if verify and hashed else 1, hashed, len(m["jobs"]), 0]


@pytest.mark.parametrize("c", [1, 64, 65, 66])
def test_candidate_counts_around_the_sorted_launch(gpu, c):
    """Exactly c candidates among 80 blocks, every third one not what its digest says."""
    kinds = [("unverified" if k % 3 == 2 else "job") for k in range(c)] + ["missing", "empty", "stale"] * 30
    kinds = kinds[:80]
    order = np.random.default_rng(c).permutation(80)
    case = pe.mixed_case(900 + c, 80, kinds=[kinds[k] for k in order])
    m = model_of(case)
    assert m["candidates"] == c and m["counts"][6] == c // 3
    x, nl = on_device(case, gpu), len(case["local_size"])
    o = outputs(80, nl, 80, gpu)
    rc, counts = call(x, o, 80, 80, gpu)
    assert (rc, counts) == (0, m["counts"]) and stats()[:2] == [2, c]
    check_outputs(o, expected_bytes(m, 80, nl, 80))


def test_300_jobs_read_one_local_file(gpu):
    case = pe.mixed_case(31, 300, kinds=("job",), n_local=1)
    m = model_of(case)
    assert m["local_jobs"] == [300]
    x = on_device(case, gpu)
    o = outputs(300, 1, 300, gpu)
    rc, counts = call(x, o, 300, 300, gpu)
    assert (rc, counts) == (0, m["counts"]) and counts[0] == 300
    check_outputs(o, expected_bytes(m, 300, 1, 300))


def test_one_changed_byte_is_unverified_with_the_arena_and_a_job_without(gpu):
    case = pe.mixed_case(32, 40, kinds=("job",), n_local=1)
    assert model_of(case)["counts"][0] == 40
    r = case["rows"][17]
    at = case["local_base"][0] + case["table_offset"][r] + case["sizes"][17] - 1  # the block's last byte
    src = bytearray(case["src"])
    src[at] ^= 0x80
    case["src"] = bytes(src)
    m, trusted = model_of(case), model_of(case, verify=False)
    assert m["cls"][17] == "unverified" and m["present"][17] == 0 and m["ask"][17] == 1
    assert trusted["cls"][17] == "job" and trusted["counts"][0] == 40
    x = on_device(case, gpu)
    for verify, want in ((True, m), (False, trusted)):
        o = outputs(40, 1, 40, gpu)
        rc, counts = call(x, o, 40, 40, gpu, verify=verify)
        assert (rc, counts) == (0, want["counts"])
        check_outputs(o, expected_bytes(want, 40, 1, 40))


@pytest.mark.parametrize("how", ["query", "query-null-outputs", "no-job-list", "cap-short", "cap-short-trusted"])
def test_a_query_and_a_short_cap_write_the_counters_alone(gpu, how):
    n = 130
    case = pe.mixed_case(41, n)
    query = how.startswith("query")
    verify = how != "cap-short-trusted"
    m = model_of(case, query=query, verify=verify)
    x, nl = on_device(case, gpu), len(case["local_size"])
    need = len(m["jobs"])
    cap = need - 1 if how.startswith("cap") else need + EXTRA
    o = outputs(n, nl, need, gpu)
    drop = {"query-null-outputs": ("present", "ask", "dst", "src_offsets", "dst_offsets", "job_sizes", "job_blocks"),
            "no-job-list": ("job_blocks",)}.get(how, ())
    rc, counts = call(x, o, n, cap, gpu, query=query, verify=verify, drop=drop)
    assert (rc, counts) == (_lib.SF_ENOSPC, m["counts"])
    check_outputs(o, expected_bytes(m, n, nl, need, lists=False))
    assert stats() == [2 if verify and not query else 1, m["candidates"], need, int(query or bool(drop))]
    # the counters are optional too
    o = outputs(n, nl, need, gpu)
    rc, counts = call(x, o, n, cap, gpu, query=query, verify=verify, drop=drop + ("local_jobs",))
    assert (rc, counts) == (_lib.SF_ENOSPC, m["counts"])
    check_outputs(o, {k: np.full(v.numel(), FILL, np.uint8) for k, v in o.items()})


@pytest.mark.parametrize("what", ["row", "file", "section", "dst", "arena"])
def test_bad_input_is_refused_with_nothing_written(gpu, what):
    n = 70
    case = pe.mixed_case(51, n)
    m = model_of(case)
    job = m["jobs"][-1][3]
    r = case["rows"][job]
    if what == "row":
        case["rows"][64] = len(case["table_file"]) if case["rows"][64] >= 0 else len(case["table_file"]) + 5
    elif what == "file":
        case["table_file"][r] = len(case["local_size"])
    elif what == "section":
        case["block_file"][-1] = len(case["file_base"])
    elif what == "dst":
        case["file_base"][1] = pe.U64 - case["offsets"][-1]
    else:
        end = max(case["local_base"][case["table_file"][case["rows"][i]]] + case["table_offset"][case["rows"][i]]
                  + case["sizes"][i] for i, c in enumerate(m["cls"]) if c in ("job", "unverified"))
        case["src"] = case["src"][:end - 1]
    assert model_of(case) == pe.ERANGE
    x, nl = on_device(case, gpu), len(case["local_size"])
    o = outputs(n, nl, n, gpu)
    rc, counts = call(x, o, n, n, gpu)
    assert (rc, counts) == (_lib.SF_ERANGE, [77] * 8)
    check_outputs(o, {k: np.full(v.numel(), FILL, np.uint8) for k, v in o.items()})
    if what == "arena":  # without the arena nothing is read from it: the plan stands
        rc, counts = call(x, o, n, n, gpu, verify=False)
        assert (rc, counts) == (0, model_of(case, verify=False)["counts"])


def test_the_edges_of_the_sums_are_accepted(gpu):
    """The destination sum at 2^64 - 1, and a candidate whose last byte is the arena's last."""
    n = 70
    case = pe.mixed_case(51, n)
    m = model_of(case)
    case["file_base"][1] = pe.U64 - 1 - case["offsets"][-1]
    end = max(case["local_base"][case["table_file"][case["rows"][i]]] + case["table_offset"][case["rows"][i]]
              + case["sizes"][i] for i, c in enumerate(m["cls"]) if c in ("job", "unverified"))
    case["src"] = case["src"][:end]
    m = model_of(case)
    assert m != pe.ERANGE and m["dst"][-1] == pe.U64 - 1
    x, nl = on_device(case, gpu), len(case["local_size"])
    o = outputs(n, nl, n, gpu)
    rc, counts = call(x, o, n, n, gpu)
    assert (rc, counts) == (0, m["counts"])
    check_outputs(o, expected_bytes(m, n, nl, n))


def test_no_blocks_clear_the_counters_and_launch_nothing_else(gpu):
    case = pe.mixed_case(5, 0)
    x = on_device(case, gpu)
    o = outputs(0, 3, 0, gpu)
    rc, counts = call(x, o, 0, 0, gpu)
    assert (rc, counts) == (0, [0] * 8) and stats() == [0, 0, 0, 0]
    want = {k: np.full(v.numel(), FILL, np.uint8) for k, v in o.items()}
    want["local_jobs"][:12] = 0
    check_outputs(o, want)


def test_the_wrapper_and_the_copy_kernel_carry_the_plan_out(gpu):
    """device.plan_copies' lists through sf_copy_blocks_device into the
    images: d_status stays 0 and the allocation is the model's jobs, byte for
    byte, with every other byte as it was."""
    n = 500
    case = pe.mixed_case(61, n)
    m = model_of(case)
    x = on_device(case, gpu)
    args = [x[k] for k in ("digests", "sizes", "offsets", "rows", "block_file", "file_base", "table_file",
                           "table_offset", "table_size", "local_size")]
    query = device.plan_copies(*args)
    assert query.present is None and query.local_jobs.cpu().tolist() == model_of(case, query=True)["local_jobs"]
    plan = device.plan_copies(*args, x["local_base"], x["src"])
    assert tuple(plan.counts) == tuple(m["counts"]) and plan.counts.jobs == len(m["jobs"]) > 50
    assert plan.present.cpu().tolist() == m["present"] and plan.ask.cpu().tolist() == m["ask"]
    assert plan.dst.cpu().tolist() == m["dst"] and plan.local_jobs.cpu().tolist() == m["local_jobs"]
    assert plan.job_blocks.cpu().tolist() == [j[3] for j in m["jobs"]]
    size = case["file_base"][1] + sum(s for s, f in zip(case["sizes"], case["block_file"]) if f == 1)
    image = torch.full((size,), 0x11, dtype=torch.uint8, device=gpu)
    status = torch.zeros(1, dtype=torch.int32, device=gpu)
    rc = _lib.lib().sf_copy_blocks_device(x["src"].data_ptr(), x["src"].numel(), image.data_ptr(), size,
                                          plan.src_offsets.data_ptr(), plan.dst_offsets.data_ptr(),
                                          plan.sizes.data_ptr(), None, plan.counts.jobs, status.data_ptr(),
                                          torch.cuda.current_stream(gpu).cuda_stream)
    assert rc == 0 and int(status.item()) == 0
    want = np.full(size, 0x11, np.uint8)
    src = np.frombuffer(case["src"], np.uint8)
    for s, d, z, _i in m["jobs"]:
        want[d:d + z] = src[s:s + z]
    assert np.array_equal(image.cpu().numpy(), want)


def test_the_call_keeps_its_callers_stream_order(gpu):
    """Every input sits behind a hold on a fresh stream and holds a decoy
    until it ends -- no block found, an arena of zeros -- and the outputs are
    allocated and read on that stream."""
    n = 300
    case = pe.mixed_case(71, n)
    m = model_of(case)
    real = on_device(case, gpu)
    decoy = {k: torch.zeros_like(v) for k, v in real.items()}
    decoy["rows"].fill_(-1)
    names = ("digests", "sizes", "offsets", "rows", "block_file", "file_base", "table_file", "table_offset",
             "table_size", "local_size", "local_base", "src")

    def run(x, s):
        p = device.plan_copies(*[x[k] for k in names], stream=s)
        return (p.present, p.ask, p.dst, p.src_offsets, p.dst_offsets, p.sizes, p.job_blocks, p.local_jobs,
                tuple(p.counts))
    H = so.hold_ms(so.timed_ms(lambda: run(real, None), gpu))
    torch.cuda.synchronize(gpu)
    S = so.fresh_stream(gpu)
    x, _o = so.pending(S, real, decoy, H)
    with torch.cuda.stream(S):
        result = run(x, S)
    got = so.settle(S, x, decoy, result)
    col = lambda k, t: np.array([j[k] for j in m["jobs"]], t)  # noqa: E731
    want = (np.array(m["present"], np.uint8), np.array(m["ask"], np.uint8), np.array(m["dst"], np.uint64),
            col(0, np.uint64), col(1, np.uint64), col(2, np.uint32), col(3, np.int64),
            np.array(m["local_jobs"], np.uint32), tuple(m["counts"]))
    assert so.same(got, want), so.first_difference(got, want)
