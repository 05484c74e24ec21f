"""GPU: the library's entry points are wired to the state table of a resident batch (DESIGN.md
section 3, csrc/batch_state.h).  One batch walks one sequence of calls; each is either accepted or
raises ValueError (VH_ERR_ARG) as the table says.  The numbers are the business of the feature tests;
tests/test_batch_state.py checks the table itself on the CPU."""
import numpy as np
import pytest

from vent_analysis_amd import _lib
from vent_analysis_amd.sphere import compact_table_for

import mask_edit_ref as M

pytestmark = pytest.mark.gpu

VOX = (1.5, 1.5, 10.0)
SHAPE = (41, 37, 9)
N = 2


def volumes():
    """As test_gpu_mask_edit.volumes: signal inside the mask, background outside."""
    rng = np.random.default_rng(11)
    hp = (rng.random((4,) + SHAPE, dtype=np.float32) * 100 + 5).astype(np.float32)
    hp *= 0.25 + (M.batch_masks(SHAPE) != 0)
    return hp[:N]


class Walk:
    """The batch and every reader of it as a named call."""

    def __init__(self):
        self.B = _lib.Batch(*SHAPE, N)
        self.table = compact_table_for(VOX, 12, SHAPE)     # a small sphere table: 12 mm
        self.parula = np.linspace(0.0, 1.0, 64 * 3).reshape(64, 3)
        self.image_bytes = 1
        B = self.B
        self.calls = {
            "download": B.download,
            "download_defect": B.download_defect,
            "select_mean": lambda: B.select_defect("mean"),
            "overlay": B.overlay,
            "montage_layout": B.montage_layout,
            "montage": self.montage,
            "distribution": lambda: B.distribution("p99", 64, 1.5),
            "select_kmeans": lambda: B.select_defect("kmeans"),
            "download_defect_km": lambda: B.download_defect(km=True),
            "km_cuts": B.km_cuts,
            "ci": lambda: B.ci(VOX, table=self.table),
            "download_ci": B.download_ci,
            "download_overlay": self.download_overlay,
            "download_montage": self.download_montage,
            "download_distribution": B.download_distribution,
        }

    NEED_RUN = ("download", "download_defect", "select_mean", "overlay", "montage_layout", "montage",
                "distribution")
    NEED_KMEANS = ("select_kmeans", "download_defect_km", "km_cuts")
    RENDER_DOWNLOADS = ("download_overlay", "download_montage", "download_distribution")

    def montage(self):
        """The enqueue alone (Batch.montage asks for the layout first, which has a guard of its own)."""
        self.B.ctx.check(self.B.L.vh_batch_montage(self.B.h, None, _lib._ptr(self.parula), len(self.parula)),
                         "vh_batch_montage")
        self.image_bytes = max(1, int(self.B.montage_layout()[1][-1]))

    def download_overlay(self):
        n, R, C, Z = self.B.shape
        out = np.empty((n, Z, R, C, 3), np.uint8)
        self.B.ctx.check(self.B.L.vh_batch_download_overlay(self.B.h, _lib._ptr(out)), "vh_batch_download_overlay")

    def download_montage(self):
        buf, status = np.empty(self.image_bytes, np.uint8), np.zeros(N, np.int32)
        self.B.ctx.check(self.B.L.vh_batch_download_montage(self.B.h, _lib._ptr(buf), _lib._ptr(status)),
                         "vh_batch_download_montage")

    def accepts(self, *names):
        for name in names:
            self.calls[name]()

    def refuses(self, *names):
        for name in names:
            with pytest.raises(ValueError):
                self.calls[name]()
                pytest.fail(f"{name} was accepted")

    def run(self, do_kmeans):
        self.B.run(self.B.options(do_n4=False, do_kmeans=do_kmeans, vox=VOX))


def test_calls_are_accepted_and_refused_as_the_state_table_says():
    w = Walk()
    B = w.B
    masks = M.batch_masks(SHAPE)[:N]
    defect = (np.random.default_rng(7).random((N,) + SHAPE) < 0.2).astype(np.uint8)

    # 1. an upload alone: every reader refuses
    B.upload(volumes(), masks)
    w.refuses(*w.NEED_RUN, *w.NEED_KMEANS, "ci", "download_ci", *w.RENDER_DOWNLOADS)

    # 2. an uploaded defect map serves the CI; nothing that needs a run
    B.upload_defect(defect)
    w.accepts("ci", "download_ci")
    w.refuses(*w.NEED_RUN, *w.NEED_KMEANS, *w.RENDER_DOWNLOADS)

    # 3. a run without k-means: the k-means calls refuse, the rest accept
    w.run(do_kmeans=False)
    w.refuses(*w.NEED_KMEANS)
    w.accepts("download", "download_defect", "select_mean", "montage_layout", "download_ci")
    w.refuses(*w.RENDER_DOWNLOADS)

    # 4. the renderings, the distribution and the CI, and their downloads
    w.accepts("overlay", "montage", "distribution", "ci")
    w.accepts(*w.RENDER_DOWNLOADS, "download_ci")

    # 5. a new run (with k-means) discards the renderings and the distribution; the CI is still there
    w.run(do_kmeans=True)
    w.refuses(*w.RENDER_DOWNLOADS)
    w.accepts("download_ci")

    # 6. the k-means selection and its labels
    w.accepts("select_kmeans", "download_defect_km", "km_cuts")

    # 7. a denoise, 9. a mask edit: what needs a run refuses, the CI calls stay; 8. a run brings all back
    for edit in (lambda: B.denoise(sigma=5.0), lambda: B.edit_mask("erode", 1)):
        edit()
        w.refuses(*w.NEED_RUN, *w.NEED_KMEANS, *w.RENDER_DOWNLOADS)
        w.accepts("download_ci", "ci")
        w.run(do_kmeans=True)
        w.accepts(*w.NEED_RUN, *w.NEED_KMEANS, "ci", "download_ci", *w.RENDER_DOWNLOADS)
    B.close()
