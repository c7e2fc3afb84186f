"""CPU: the strict operand check the opt-in gradient bindings share (zest_hip._strict_operands, _strict_buffer,
_strict_devices) on its own: every refusal, in the order given, buffers after operands, devices last."""
import pytest
import torch


def test_operands_then_buffers_then_devices():
    import zest_hip as zh
    a, b = torch.zeros(3, 5, 8), torch.zeros(2, 8)
    ops = lambda a=a, b=b: [("a", a, "[N,M,8]", lambda t: t.dim() == 3 and t.shape[2] == 8), ("b", b, (2, None))]
    assert zh._strict_operands("who", ops()) is None                 # nothing about devices yet: CPU tensors pass
    sentence = "who: %s must be a contiguous fp32 tensor %s, got .*%s"
    for bad, got in ((None, "NoneType"), (3.0, "float"), (a.double(), r"torch.float64 \(3, 5, 8\), contiguous: True"),
                     (a.to(torch.bfloat16), "torch.bfloat16"), (torch.zeros(3, 8, 5).transpose(1, 2), "contiguous: False"),
                     (torch.zeros(3, 5, 16)[..., ::2], "contiguous: False"), (a[0], r"\(5, 8\)"), (torch.zeros(3, 5, 7), r"\(3, 5, 7\)")):
        with pytest.raises(RuntimeError, match=sentence % ("a", r"\[N,M,8\]", got)):
            zh._strict_operands("who", ops(a=bad))
    for bad, got in ((None, "NoneType"), (b.half(), "torch.float16"), (torch.zeros(8, 2).t(), "contiguous: False"),
                     (torch.zeros(3, 8), r"\(3, 8\)"), (b[0], r"\(8,\)"), (b[None], r"\(1, 2, 8\)")):
        with pytest.raises(RuntimeError, match=sentence % ("b", r"\(2, '\*'\)", got)):
            zh._strict_operands("who", ops(b=bad))
    with pytest.raises(RuntimeError, match="who: a must be"):        # in the order given: the first bad operand speaks
        zh._strict_operands("who", ops(a=a.double(), b=None))
    # a caller's buffer: dtype, element count or shape, contiguity, alignment where asked - and nothing about its device
    work = torch.zeros(40)
    assert zh._strict_buffer("who", "work", work, a, 40, aligned=True) is work
    out = zh._strict_buffer("who", "out", None, a, (3, 4))           # none given: a fresh one beside `like`
    assert tuple(out.shape) == (3, 4) and out.dtype == torch.float32 and out.device == a.device
    assert zh._strict_buffer("who", "work", None, a, 24, torch.uint8).dtype == torch.uint8
    for bad in (3, work.double(), torch.zeros(39), torch.zeros(80)[::2], torch.zeros(44)[1:41]):
        with pytest.raises(RuntimeError, match="who: work must be 40 contiguous fp32 elements, 16-byte aligned"):
            zh._strict_buffer("who", "work", bad, a, 40, aligned=True)
    assert zh._strict_buffer("who", "work", torch.zeros(44)[1:41], a, 40).data_ptr() % 16 == 4      # alignment only where asked
    for bad in (torch.zeros(12), torch.zeros(4, 3).t(), torch.zeros(3, 4, dtype=torch.int32)):
        with pytest.raises(RuntimeError, match=r"who: out must be a contiguous fp32 tensor \(3, 4\)$"):
            zh._strict_buffer("who", "out", bad, a, (3, 4))
    with pytest.raises(RuntimeError, match="who: work must be 24 contiguous uint8 elements$"):
        zh._strict_buffer("who", "work", work, a, 24, torch.uint8)
    # devices last, operands before buffers, everything on the first operand's
    with pytest.raises(RuntimeError, match=r"who: a is on cpu; this path runs only on a HIP device \(all tensors on one\)"):
        zh._strict_devices("who", ops(), work=work)
    with pytest.raises(RuntimeError, match="who: b is on cpu"):
        zh._strict_devices("who", [("a", _Hip(a)), ("b", b)], work=work)
    with pytest.raises(RuntimeError, match="who: work is on cpu"):
        zh._strict_devices("who", [("a", _Hip(a)), ("b", _Hip(b))], out=_Hip(out), work=work)
    with pytest.raises(RuntimeError, match="who: out is on meta"):
        zh._strict_devices("who", [("a", _Hip(a))], out=_Hip(out.to("meta")))             # not the first operand's
    assert zh._strict_devices("who", [("a", _Hip(a)), ("b", _Hip(b))], work=_Hip(work)) == a.device


class _Hip:
    """A tensor that says it is on a HIP device: what _strict_devices asks of one, and no more."""

    def __init__(self, t):
        self.device, self.is_cuda = t.device, True
