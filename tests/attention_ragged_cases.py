"""Cases of tests/test_gpu_attention_ragged.py and the mirror of the host dispatch of csrc/attention_ragged.hip
(advh_attention_f16_ragged, advh_attention_split_ragged), free of GPU imports so that
tests/test_build_resources_attention_ragged.py can hold the cases against the compiled instances.

The ragged entry points pick their kernel by the row STRIDE T exactly as the siblings do by T, so the mirror is
attention_kernel_cases.instance_of with the kernel renamed."""
import attention_kernel_cases as K

ENTRIES = K.ENTRIES
STRIDES = (16, 64, 65, 128, 129, 208, 209, 256)          # both edges of every tile-count class that has more than one frame
STREAM_STRIDES = (112, 113, 225)                         # the streaming kernel's key blocks of 112: one, two, three
HEAD_DIMS = (24, 32, 56, 64, 72, 120, 128)
STREAM_DIMS = (72, 120, 128)
B, HEADS = 3, 2
SIBLING = {"attention_ragged_kernel": "attention_kernel", "attention_ragged_tr_kernel": "attention_tr_kernel",
           "attention_ragged_x3_kernel": "attention_x3_kernel", "attention_ragged_x3_tr_kernel": "attention_x3_tr_kernel",
           "attention_ragged_x3_stream_kernel": "attention_x3_stream_kernel"}
RAGGED = {v: k for k, v in SIBLING.items()}
F16 = ("attention_ragged_tr_kernel", "attention_ragged_kernel")
SPLIT = ("attention_ragged_x3_tr_kernel", "attention_ragged_x3_kernel", "attention_ragged_x3_stream_kernel")


def instance_of(entry, T, dm):
    """(kernel, template arguments ...) launched for row stride ``T`` and head dim ``dm``."""
    inst = K.compiled_name(K.instance_of(entry, T, dm))
    return (RAGGED[inst[0]],) + inst[1:]


def middle(T, stream=False):
    """Valid frames of the third clip.  Streaming cases: at the 112-key block edge (111 | 112 | 113 for strides 112 | 113 | 225:
    one key short of a block, one whole block under a two-block stride, one key into the second block).  Otherwise at a 16-frame
    tile edge: one frame into a tile -- T - 15 where the stride is a whole number of tiles, 17 elsewhere."""
    if stream:
        return {112: 111, 113: 112, 225: 113}[T]
    return T - 15 if T % 16 == 0 else 17


def frames_of(T, stream=False):
    return (T, 1, middle(T, stream))


def _cases():
    out = [(entry, T, HEADS, dm, B, False) for T in STRIDES for dm in HEAD_DIMS for entry in ENTRIES]
    return out + [("split", T, HEADS, dm, B, True) for T in STREAM_STRIDES for dm in STREAM_DIMS]


CASES = _cases()                                         # (entry, T, heads, dm, B, stream case)


def case_id(c):
    return "{}-T{}-h{}-d{}-B{}{}".format(*c[:5], "-blocks" if c[5] else "")


def selected(cases=None):
    sel = {}
    for c in (CASES if cases is None else cases):
        sel.setdefault(instance_of(c[0], c[1], c[3]), []).append(c)
    return sel
