"""The table of tests/test_containment_gpu.py is closed over include/maua_hip.h: every declared entry point that takes a non-const pointer
(something it may write through) is named by a case, or by EXEMPT with the one admissible reason - it writes no device memory.  An entry
point added to the header later fails here until it has a case.  Needs no GPU and no library; the guard-band helper is checked on the CPU."""
import os
import re

import torch

import test_containment_gpu as cg
from conftest import REPO
from guarded import GUARD_MIN, Guarded

HEADER = os.path.join(REPO, "include", "maua_hip.h")


def declarations(text):
    """name -> list of parameter strings of every function the header declares."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = "\n".join(line for line in text.splitlines() if not line.lstrip().startswith("#"))
    out = {}
    for m in re.finditer(r"\b(maua_\w+)\s*\(([^()]*)\)\s*;", text):
        out[m.group(1)] = [p.strip() for p in m.group(2).split(",") if p.strip() and p.strip() != "void"]
    return out


def writes_through(param):
    """A pointer parameter whose pointee is not const: `float* y`, `void* workspace`, `float* const* grams` - not `const float* x`,
    `const void* const* workspaces`, nor the stream handle (no pointer in its spelling)."""
    return "*" in param and not param.startswith("const ")


def writers():
    with open(HEADER) as f:
        decl = declarations(f.read())
    assert len(decl) > 100 and "maua_conv3x3_x3w" in decl and "maua_nca_grad_finish" in decl
    return decl, {name for name, params in decl.items() if any(writes_through(p) for p in params)}


def test_parser_tells_outputs_from_inputs():
    decl, w = writers()
    assert "maua_relu_fwd" in w and "maua_gram_finish_mse_batch" in w and "maua_conv_arm_workspace" in w and "maua_lbfgs_init" in w
    for reads_only in ("maua_last_error", "maua_conv_x3w_bank_bytes", "maua_set_tuning", "maua_get_tuning", "maua_abi_version", "maua_flow_levels"):
        assert reads_only in decl and reads_only not in w
    assert [p for p in decl["maua_lbfgs_status"] if writes_through(p)] == ["float* out5"]


def test_every_entry_point_that_can_write_has_a_case():
    decl, w = writers()
    named = cg.declared_entry_points()
    unknown = sorted((named | set(cg.EXEMPT)) - set(decl))
    assert not unknown, f"the table names entry points the header does not declare: {unknown}"
    uncovered = sorted(w - named - set(cg.EXEMPT))
    assert not uncovered, f"entry points that take a non-const pointer and have no containment case (tests/test_containment_gpu.py): {uncovered}"
    both = sorted(named & set(cg.EXEMPT))
    assert not both, f"exempt and covered at once: {both}"
    for name, reason in cg.EXEMPT.items():
        assert "writes no device memory" in reason, (name, reason)


def test_case_ids_are_unique_and_every_case_names_entry_points():
    ids = [c.id for c in cg.TABLE]
    assert len(ids) == len(set(ids))
    assert all(c.entries and all(e.startswith("maua_") for e in c.entries) for c in cg.TABLE)


def test_guard_band_layout_and_damage_report():
    """tests/guarded.py on the CPU: back guard at the byte behind the payload, front guard a multiple of 256 bytes, both at least
    max(1 MiB, 2 x payload); a changed byte is reported relative to the payload's end."""
    for shape, dtype in (((3, 5), torch.float32), ((1,), torch.float64), ((700001,), torch.uint8), ((0,), torch.float32)):
        g = Guarded(shape, dtype, device="cpu")
        need = max(GUARD_MIN, 2 * g.nbytes)
        assert g.front % 256 == 0 and g.front >= need and g.back >= need and g.buf.numel() == g.front + g.nbytes + g.back
        assert (g.payload.data_ptr() if g.nbytes else g.ptr()) == g.buf.data_ptr() + g.front and tuple(g.payload.shape) == tuple(shape) and g.payload.dtype == dtype
        assert bool((g.payload_bytes == 0xFF).all()) and g.intact()
        g.payload_bytes.fill_(0)                           # writing the whole payload touches no guard
        assert g.intact()
        g.buf[g.front + g.nbytes] = 0                      # one byte past the end
        g.buf[g.front + g.nbytes + 300] = 1
        assert g.damage() == dict(first=0, last=300, changed=2, payload_bytes=g.nbytes)
        g.buf[g.front - 1] = 0                             # and the byte in front of the payload
        assert g.damage()["first"] == -g.nbytes - 1 and not g.intact()
    t = torch.arange(6, dtype=torch.float32).reshape(2, 3)
    g = Guarded.of(t, guard_fill=0xFF, device="cpu")
    assert torch.equal(g.payload, t) and bool((g.buf[:g.front] == 0xFF).all()) and bool((g.buf[g.front + g.nbytes:] == 0xFF).all())
