"""MI355X-native Conv-TasNet hot path (gfx950 HIP kernels behind a C ABI, PyTorch-ROCm as plumbing).

Drop-in surfaces of the reference kept here: ``ConvTasNet``, ``cal_loss``, ``overlap_and_add``,
``Solver``, ``separate``.  Import name: ``conv_tasnet_amd``.
"""
from ._lib import lib, CtnError, LIB_PATH  # noqa: F401
from .conv_tasnet import ConvTasNet  # noqa: F401
from .pit_criterion import cal_loss, cal_si_snr_with_pit  # noqa: F401
from .utils import overlap_and_add, remove_pad  # noqa: F401
from .ops import gemm_arith, gemm_arithmetic, set_gemm_arith  # noqa: F401
from .streaming import StreamingSeparator, FusedStreamingSeparator, FusedStreamPool, ResamplingStreamPool  # noqa: F401
from .dynmix import DeviceCorpus, DynamicMixLoader  # noqa: F401
from . import resample  # noqa: F401
from .resample import StreamResampler  # noqa: F401
from . import rir  # noqa: F401
from .rir import RirBank  # noqa: F401
from . import longform  # noqa: F401
from .longform import separate_long, frame_ragged, stitch_ragged, plan_segments, fade_tables  # noqa: F401
from .stoi import StoiPitCriterion, cal_stoi_loss, stoi, stoi_batch, stoi_both, stoi_improvement, stoi_pairs  # noqa: F401  (ctn.stoi is the function; the module: conv_tasnet_amd.stoi)
from . import mrstft  # noqa: F401
from .mrstft import MrStftPitCriterion, cal_mrstft_loss, mrstft_pairs  # noqa: F401
from . import mixit  # noqa: F401
from .mixit import cal_mixit_loss, remix, pair_batch, MixtureOfMixtures, MixItCriterion  # noqa: F401
from . import varpit  # noqa: F401
from .varpit import cal_varpit_loss, VarPitCriterion, output_levels, count_sources, evaluate_variable  # noqa: F401
from . import assign  # noqa: F401
from .assign import cal_assign_loss, linear_assignment, reorder_estimate, AssignPitCriterion  # noqa: F401

__version__ = "0.1.0"
