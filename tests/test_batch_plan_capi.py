"""C-ABI and binding of the full-horizon plan (srbd_batch_plan_device, srbd_batch_plan, srbd_plan, srbd_batch_plan_io,
include/srbd_mpc.h; BatchContext.plan_device / plan, Context.plan).  CPU only: every check here is decided before a
device call.  The two refusals that need a batch's horizon and gait setting (contact_stride < H, freqs NULL) are made
here by the binding on a hollow batch, and by the C function on a live batch in tests/test_gpu_batch_plan.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from quadruped_pympc_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "srbd_mpc.h")
INPUTS = ("states", "refs", "contacts", "params", "freqs")
OUTPUTS = _lib.PLAN_OUTPUTS


def fake_io(**over):
    io = _lib.BatchPlanIO()
    for name in INPUTS + OUTPUTS:
        setattr(io, name, 0x1000)
    io.contact_stride = 12
    for k, v in over.items():
        setattr(io, k, v)
    return io


def last_error():
    msg = _lib.lib.srbd_batch_last_error(None)
    return msg.decode() if msg else ""


def test_exports_and_abi_version():
    for name in ("srbd_batch_plan_device", "srbd_batch_plan", "srbd_plan"):
        assert name in _lib.SIGNATURES
        assert getattr(_lib.lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert _lib.lib.srbd_abi_version() == 1
    assert callable(_lib.BatchContext.plan_device) and callable(_lib.BatchContext.plan) and callable(_lib.Context.plan)


def test_struct_layout_matches_header():
    text = open(HEADER).read()
    body = re.search(r"typedef struct srbd_batch_plan_io \{(.*?)\} srbd_batch_plan_io;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(?:const\s+)?(\w+)\s*(\*?)\s*(.+)$", decl)
        for name in m.group(3).split(","):
            assert m.group(2) or m.group(1) == "int32_t", decl
            fields.append((name.strip(), bool(m.group(2))))
    assert [f[0] for f in fields] == [f[0] for f in _lib.BatchPlanIO._fields_]
    size = 0
    for name, is_ptr in fields:
        width = 8 if is_ptr else 4
        size = (size + width - 1) // width * width
        assert getattr(_lib.BatchPlanIO, name).offset == size, name
        size += width
    assert C.sizeof(_lib.BatchPlanIO) == (size + 7) // 8 * 8 == 8 * 10 + 2 * 4


def test_null_io_and_null_batch():
    lib = _lib.lib
    assert lib.srbd_batch_plan_device(None, None, None) == _lib.E_INVALID
    assert "null io" in last_error()
    assert lib.srbd_batch_plan_device(None, C.byref(fake_io()), None) == _lib.E_INVALID
    assert "null batch" in last_error()
    assert lib.srbd_plan(None, *([None] * 3), 12, None, 0.0, *([None] * 5)) == _lib.E_INVALID
    assert "null context" in (_lib.lib.srbd_last_error(None) or b"").decode()
    assert lib.srbd_batch_plan(None, *([None] * 3), 12, *([None] * 7)) == _lib.E_INVALID


@pytest.mark.parametrize("field", ("states", "refs", "params"))
def test_null_required_pointer_is_named(field):
    assert _lib.lib.srbd_batch_plan_device(None, C.byref(fake_io(**{field: None})), None) == _lib.E_INVALID
    assert last_error().endswith("null required pointer: " + field)


def test_every_output_null_is_refused_and_any_one_passes():
    none = {k: None for k in OUTPUTS}
    assert _lib.lib.srbd_batch_plan_device(None, C.byref(fake_io(**none)), None) == _lib.E_INVALID
    assert "every output is NULL" in last_error()
    for keep in OUTPUTS:  # one output is enough: the call goes on to refuse the null batch
        io = fake_io(**{k: None for k in OUTPUTS if k != keep})
        assert _lib.lib.srbd_batch_plan_device(None, C.byref(io), None) == _lib.E_INVALID
        assert "null batch" in last_error()


# ------------------------------------------------------------------ the binding's checks, before the C call
E, N, H, P = 3, 100, 12, 144


@pytest.fixture
def hollow_batch(monkeypatch):
    calls = []
    monkeypatch.setattr(_lib.lib, "srbd_batch_plan_device", lambda *a: calls.append(a) or _lib.OK)
    b = _lib.BatchContext.__new__(_lib.BatchContext)
    b.E, b.N, b.P, b.h = E, N, P, None
    b.cfg = _lib.make_config(num_samples=N, horizon=H, method="mppi", parametrization="zero_order", mass=15.0,
                             inertia=np.eye(3), dts=np.full(H, 0.02))
    return b, calls


def good_args():
    return dict(states=torch.zeros(E, 24), refs=torch.zeros(E, 24), contacts=torch.ones(E, 4, H),
                params=torch.zeros(E, P))


BAD = [
    ("contacts", lambda: torch.ones(E, 4, H - 1), "contacts"),  # contact_stride < H
    ("contacts", lambda: None, "contacts"),
    ("states", lambda: torch.zeros(E - 1, 24), "must be"),
    ("refs", lambda: torch.zeros(E, 24, dtype=torch.float64), "float32"),
    ("params", lambda: torch.zeros(E, P + 12), "must be"),
    ("params", lambda: np.zeros((E, P), np.float32), "torch tensor"),
    ("freqs", lambda: torch.zeros(E + 1), "must be"),
]


@pytest.mark.parametrize("name,make,match", BAD, ids=[f"{i}_{b[0]}" for i, b in enumerate(BAD)])
def test_plan_device_refuses_bad_tensors_before_the_c_call(hollow_batch, name, make, match):
    b, calls = hollow_batch
    kw = good_args()
    kw[name] = make()
    with pytest.raises(ValueError, match=match):
        b.plan_device(**kw)
    assert not calls


def test_plan_device_needs_freqs_with_gait_and_a_known_output(hollow_batch):
    b, calls = hollow_batch
    b._gait = True
    with pytest.raises(ValueError, match="freqs is required"):
        b.plan_device(**good_args())
    b._gait = False
    with pytest.raises(ValueError, match="want must name"):
        b.plan_device(**good_args(), want=())
    with pytest.raises(ValueError, match="want must name"):
        b.plan_device(**good_args(), want=("plan_cost", "grf"))
    with pytest.raises(ValueError, match="must be on cuda:0"):
        b.plan_device(**good_args())
    assert not calls
