"""The selectable kernel forms of the two GEMM families, as (id, name) lists: what the `gemm_shape` and `tn_variant` fixtures of
test_kernels_gpu.py and test_gemm_small_shapes_gpu.py are parametrised over.  One list, so that the two files cannot drift apart.

NT_SHAPES are the ids of oneprot_gemm_force_shape (include/oneprot_hip.h), TN_VARIANTS those of oneprot_gemm_tn_variant; -1 is the library's own choice."""

NT_SHAPES = [(-1, "auto"), (0, "128x128"), (1, "256x128"), (2, "256x256"), (3, "128x128bk64"), (4, "256x256bk64"), (5, "256x256nopipe"), (6, "4w128x128bk64"),
             (7, "4w128x128bk32"), (8, "regstaged256x256"), (17, "direct256x128"), (19, "direct128x128bk64"), (20, "direct256x256bk64"), (32, "pingpong"),
             (40, "8phase256x256"), (41, "8phase256x320"), (42, "8phase256x256merged")]

TN_VARIANTS = [(-1, "auto"), (0, "dma64x2"), (1, "dma32x3"), (2, "regstaged"), (3, "8phase")]


def ids(forms):
    return [i for i, _ in forms]


def names(forms):
    return [n for _, n in forms]
