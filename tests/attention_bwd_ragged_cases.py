"""Cases of tests/test_gpu_attention_bwd_ragged.py and the mirror of the host dispatch of advh_attention_bwd_f16_ragged
(csrc/backward.hip) and advh_attention_bwd_split_ragged (csrc/attention_bwd_f32.hip, csrc/attention_bwd_x3.hip), free of GPU
imports so that tests/test_build_resources_attention_bwd_ragged.py can hold the cases against the compiled instances.

The ragged kernels are the RAGGED = true instances of the batch kernels' templates (the siblings: the same template arguments
with RAGGED = false), and the ragged entry points pick theirs by the row STRIDE T exactly as the batch ones do by T, so the
mirror is backward_kernel_cases.instance_of with the last argument set."""
import backward_kernel_cases as K

ENTRIES = K.ENTRIES                                       # "f16" | "split" | "split_f32" (attention_bwd_mfma_f32 = 1)
STRIDES = (16, 64, 65, 128, 129, 208, 209, 256)           # both edges of every tile-count class, in whole strides
HEAD_DIMS = (24, 56, 64, 120)                             # D = 32, 64 (padded), 64 (exact: the transposing-read path), 128
B, HEADS = 3, 2
SOURCES = {"attention_bwd_kernel": "backward.hip", "attention_bwd_x3_kernel": "attention_bwd_x3.hip",
           "attention_bwd_f32_kernel": "attention_bwd_f32.hip"}
CLASSES = {4: (16, 64), 8: (65, 128), 13: (129, 208), 16: (209, 256)}


def instance_of(entry, T, dm):
    """(kernel, NT, D, TR | NW, True) launched for row stride ``T`` and head dim ``dm``."""
    return K.instance_of("f16" if entry == "f16" else "split", T, dm, entry == "split_f32", ragged=True)


def sibling(inst):
    """The batch instance of the same template arguments."""
    return inst[:-1] + (False,)


def middle(T):
    """Valid frames of the third clip: one frame into a 16-frame tile -- T - 15 where the stride is a whole number of tiles, 17
    elsewhere."""
    return T - 15 if T % 16 == 0 else 17


def frames_of(T):
    return (T, 1, middle(T))


def _cases():
    out = []
    for T in STRIDES:
        for dm in HEAD_DIMS:
            for entry in ENTRIES:
                if entry == "split_f32" and dm > 64:
                    continue                              # head dims > 64 run the fp32-MFMA kernel by default ("split")
                if entry == "f16" and K.refused_f16(T, dm):
                    continue                              # REFUSED
                out.append((entry, T, HEADS, dm, B))
    return out


CASES = _cases()                                          # (entry, T, heads, dm, B)
REFUSED = [(T, dm) for dm in HEAD_DIMS if dm > 64 for T in (209, 256)]


def case_id(c):
    return "{}-T{}-h{}-d{}-B{}".format(*c)


def selected(cases=None):
    sel = {}
    for c in (CASES if cases is None else cases):
        sel.setdefault(instance_of(c[0], c[1], c[3]), []).append(c)
    return sel
