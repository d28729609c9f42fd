"""The step / rollout kernels' opening, read off the built library's ISA (tools/kernarg_touch.py; no GPU): every 64-byte line of the
kernel-argument segment is requested before the first scalar wait, and exactly one wait on argument loads stands before the first
LDS-DMA state load on the fall-through path (the graph-safe `*step_ctr` dereference, a dependent load, aside).  Looks at s_load and
s_waitcnt lines only."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("kernarg_touch", os.path.join(ROOT, "tools", "kernarg_touch.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


KT = _tool()
ARG_BYTES = 1104          # DevPtrs + StepCfg + Model<double>: the three by-value arguments the kernels share


def _parsed(kernel):
    if KT.find_objdump() is None:
        pytest.skip("llvm-objdump (ROCm) not found")
    if not os.path.exists(KT.DEFAULT_LIB):
        pytest.skip("libgaq.so is not built")
    text = KT.disassemble(kernel)
    assert text is not None, "%s is not in the library" % kernel
    return KT.parse(text)


@pytest.mark.parametrize("kernel", ["step_kernel<148>", "step_kernel<276>", "rollout_kernel<20>"])
def test_one_argument_wait_before_the_first_state_load(kernel):
    res = _parsed(kernel)
    assert res["first_dma"] is not None
    assert res["waits_before_dma"]["kernarg"] == 1, res["waits_before_dma"]
    assert res["late_lines"] == [] and res["lines_after_dma"] == []
    assert sorted(res["order"])[:(ARG_BYTES + 63) // 64] == list(range((ARG_BYTES + 63) // 64))     # every line of the three structs


def test_parser_on_a_hand_written_listing():
    """The parser itself: offsets through a derived base, the three kinds of wait, late lines."""
    text = """
    <k>:
	s_load_dwordx2 s[8:9], s[0:1], 0xc0
	s_load_dwordx4 s[4:7], s[0:1], 0x108
	s_waitcnt lgkmcnt(0)
	s_load_dwordx2 s[10:11], s[8:9], 0x0
	s_waitcnt lgkmcnt(0)
	s_add_u32 s20, s0, 0x328
	s_addc_u32 s21, s1, 0
	s_load_dwordx16 s[36:51], s[20:21], 0x20
	s_waitcnt vmcnt(0) lgkmcnt(0)
	buffer_load_dwordx4 v107, s[80:83], 0 offen lds
	ds_read_b32 v1, v2
	s_waitcnt lgkmcnt(0)
	s_load_dword s3, s[0:1], 0x40
	s_waitcnt lgkmcnt(0)
    """
    res = KT.parse(text)
    assert res["order"] == [3, 4, 13, 14, 1]
    assert res["waits_before_dma"] == {"kernarg": 2, "deref": 1, "other": 0}
    assert res["late_lines"] == [13, 14, 1] and res["lines_after_dma"] == [1]
    assert [d["kind"] for _, k, d in res["events"] if k == "wait"] == ["kernarg", "deref", "kernarg", "other", "kernarg"]
