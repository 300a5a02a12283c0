"""The native rescoring session (rescore.hip) against the eager rescan, and
the pipeline with the session on and off.

The session launches the library's own featurize / GEMM / gemv kernels, so
its scores must be array-equal to the eager path's, not merely close. The
error cases provoke nothing on the device: each returns before any launch.
"""

import asyncio

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MAX_ROWS = 256   # the session under test; the default 1024 only makes buffers larger
N_SLOTS = 4


@pytest.fixture(scope="module")
def hip():
    from mcp_context_forge_amd.ops import hip as _hip

    if not _hip.available():
        pytest.fail("libforge_hip must load on a GPU box (no silent fallback)")
    return _hip


@pytest.fixture(scope="module")
def clf(hip):
    from mcp_context_forge_amd.gpu.classifier import GpuClassifier
    from mcp_context_forge_amd.models.classifier import HashedTextClassifier

    c = GpuClassifier(HashedTextClassifier(), "cuda")   # production 4096 x 1024 x 8
    assert (c.dim, c.hidden, c.classes) == (4096, 1024, 8)
    return c


@pytest.fixture()
def session(hip, clf):
    s = hip.RescoreSession(clf.w1t, clf.b1, clf.w2t, clf.b2, max_rows=MAX_ROWS, n_slots=N_SLOTS)
    yield s
    s.close()


def _texts(n, salt=0):
    out = []
    for i in range(n):
        if i == 2:
            out.append(b"")   # an empty row scores the zero vector
        else:
            out.append(('{"m":"row %d mail [EMAIL] please convert %s","n":%d}'
                        % (i + salt, "time zone " * ((i + salt) % 5), i)).encode())
    return out


def _join(texts):
    offs = np.zeros(len(texts) + 1, dtype=np.int64)
    np.cumsum([len(t) for t in texts], out=offs[1:])
    return b"".join(texts), offs.tobytes()


@pytest.fixture(scope="module")
def reference(hip, clf):
    """Eager scores per (n, salt), computed once per case and never modified."""
    from mcp_context_forge_amd.gpu.batch import pack_texts

    cache = {}

    def ref(n, salt=0):
        if (n, salt) not in cache:
            feats = hip.featurize(*pack_texts(_texts(n, salt), "cuda"), clf.dim, pad_to=128)[0]
            arr = clf.forward(feats)[:n].cpu().numpy()
            arr.setflags(write=False)
            cache[(n, salt)] = arr
        return cache[(n, salt)]

    return ref


@pytest.mark.parametrize("n", [1, 9, 64, 65, 128, MAX_ROWS])
def test_scores_equal_the_eager_rescan(session, reference, n):
    blob, offs = _join(_texts(n))
    slot = session.submit(blob, offs, n)
    assert slot >= 0
    try:
        session.wait(slot)
        assert session.poll(slot)
        got = session.scores(slot, n)
    finally:
        session.release(slot)
    assert got.shape == (n, 8) and got.dtype == np.float32
    assert np.array_equal(got, reference(n))


def test_eager_reference_is_the_same_with_the_skinny_gemm_off(hip, clf, reference, monkeypatch):
    """The reference above runs GpuClassifier.forward, which itself picks the
    64x64-tile GEMM at these sizes: pin it to the v1 kernel once."""
    from mcp_context_forge_amd.gpu.batch import pack_texts

    monkeypatch.setenv("FORGE_GEMM_SKINNY", "0")
    monkeypatch.setenv("FORGE_GEMM_V1", "1")
    feats = hip.featurize(*pack_texts(_texts(65), "cuda"), clf.dim, pad_to=128)[0]
    assert np.array_equal(clf.forward(feats)[:65].cpu().numpy(), reference(65))


def test_two_submits_outstanding(session, reference):
    a, b = _join(_texts(9)), _join(_texts(65, salt=100))
    sa = session.submit(a[0], a[1], 9)
    sb = session.submit(b[0], b[1], 65)
    assert sa >= 0 and sb >= 0 and sa != sb
    try:
        session.wait(sb)
        session.wait(sa)
        got_a, got_b = session.scores(sa, 9), session.scores(sb, 65)
    finally:
        session.release(sa)
        session.release(sb)
    assert np.array_equal(got_a, reference(9))
    assert np.array_equal(got_b, reference(65, salt=100))


def test_busy_then_free_after_release(hip, session):
    blob, offs = _join(_texts(3))
    slots = [session.submit(blob, offs, 3) for _ in range(N_SLOTS)]
    assert sorted(slots) == list(range(N_SLOTS))
    assert session.submit(blob, offs, 3) == -hip.ERR_RESCORE_BUSY
    for s in slots:
        session.wait(s)
    session.release(slots[1])
    again = session.submit(blob, offs, 3)
    assert again == slots[1]
    session.wait(again)
    for s in slots:
        session.release(s)


def test_argument_errors_return_before_any_launch(hip, session):
    blob, offs = _join(_texts(4))
    # more rows than the session holds
    many = np.zeros(MAX_ROWS + 2, dtype=np.int64).tobytes()
    assert session.submit(b"", many, MAX_ROWS + 1) == -hip.ERR_RESCORE_ARGS
    # more bytes than the session holds
    big = np.array([0, session.max_bytes + 1], dtype=np.int64).tobytes()
    assert session.submit(b"x", big, 1) == -hip.ERR_RESCORE_ARGS
    # a decreasing offset
    bad = np.frombuffer(offs, dtype=np.int64).copy()
    bad[2] = bad[1] - 1
    assert session.submit(blob, bad.tobytes(), 4) == -hip.ERR_RESCORE_ARGS
    # none of them took a slot
    got = [session.submit(blob, offs, 4) for _ in range(N_SLOTS)]
    assert sorted(got) == list(range(N_SLOTS))
    for s in got:
        session.wait(s)
        session.release(s)


def test_pipeline_responses_identical_with_session_on_and_off(monkeypatch):
    """The shape of test_pass1_graph_matches_eager: 300 rows, 200 of them
    carrying an address that the PII plugin rewrites, so the rescan runs."""
    monkeypatch.delenv("FORGE_RESCORE_NATIVE", raising=False)

    async def go():
        import os

        from mcp_context_forge_amd.config import Settings
        from mcp_context_forge_amd.engine import GatewayEngine
        from mcp_context_forge_amd.services.upstream import make_fake_time_upstream

        e = GatewayEngine(Settings(database_url="sqlite://", federation_enabled=False,
                                   auth_required=False, gpu_enabled=True))
        await e.gateway_service.register_gateway(name="t", url="inproc://t",
                                                 client=make_fake_time_upstream())
        assert e.enable_gpu()
        raws = []
        for i in range(300):
            if i % 3 == 0:
                args = '{"time":"2026-01-02T03:04:05Z","source_timezone":"UTC","target_timezone":"UTC"}'
                raws.append((f'{{"jsonrpc":"2.0","id":{i},"method":"tools/call","params":'
                             f'{{"name":"t-convert_time","arguments":{args}}}}}').encode())
            else:
                raws.append((f'{{"jsonrpc":"2.0","id":{i},"method":"tools/call","params":'
                             f'{{"name":"t-echo","arguments":{{"m":"row {i} a@b.co","n":{i}}}}}}}').encode())
        pipe = e.gpu_pipeline
        out_native = await e.process_rpc_batch(list(raws))
        st = pipe.stats()
        assert st["rescore_native"] >= 1 and st["rescore_eager"] == 0, st
        os.environ["FORGE_RESCORE_NATIVE"] = "0"
        try:
            out_eager = await e.process_rpc_batch(list(raws))
        finally:
            del os.environ["FORGE_RESCORE_NATIVE"]
        st = pipe.stats()
        assert st["rescore_eager"] >= 1, st
        assert out_native == out_eager
        await e.shutdown()

    asyncio.run(go())
