"""numpy restatement of the compact sample map the listed sampling rounds apply with the
inside-ray list (mli_sdf MLI_SDF_MODE_SDF_LISTED, mli_sample_fine with inside_list; include/mli_hip.h)
and of the dists mli_inside_list writes for the rays those rounds skip."""
import numpy as np

from inside_ref import inside_list


def sample_map(outside, n_per_ray, n_pad=0):
    """The original slot k R + r ([n_per_ray][R] layout) of every compact point ci the listed sdf
    round evaluates ([n_inside * n_per_ray] int64): sample ci % n_per_ray of ray
    inside_list[ci / n_per_ray]; compact points past them are skipped.  Any n_per_ray."""
    lst, n = inside_list(outside, n_pad)
    R = len(lst)
    ci = np.arange(n * n_per_ray, dtype=np.int64)
    return (ci % n_per_ray) * R + lst[ci // n_per_ray].astype(np.int64)


def listed_rays(outside, n_pad=0):
    """[R] bool: the rays the listed rounds work on (inside the bounds, or one of the first n_pad
    outside them)."""
    out = np.asarray(outside) != 0
    return ~out | (np.cumsum(out) <= n_pad)


def fill_dists(near, far, N):
    """dists [N][R] of the rays the listed rounds skip, fp32 operation by operation:
    min(max(near + ((k + 0.5) / N) * (far - near), near), far)."""
    near, far = np.asarray(near, np.float32), np.asarray(far, np.float32)
    t = (np.arange(N, dtype=np.float32)[:, None] + np.float32(0.5)) / np.float32(N)
    d = near[None] + (t * (far - near)[None]).astype(np.float32)
    return np.minimum(np.maximum(d.astype(np.float32), near[None]), far[None])
