"""tap-stark hot path, MI355X-native: host-side mirror of the reference's uni-stark/fri
prover interface over the C-ABI HIP library (include/tapstark.h)."""
from . import air, airs  # noqa: F401
from .air import (BaseAir, ExtExpr, LogUp, SymbolicAirBuilder, air_tape, get_log_quotient_degree,  # noqa: F401
                  get_max_constraint_degree, get_symbolic_constraints)
from .stark import (BatchLookupResult, BatchResult, BfChallenger, Blake3Mmcs, CompiledAir, Context, DeviceMatrix, FriConfig, PcsData, PinnedHostBytes, PreprocessedKey, PinnedHostMatrix,  # noqa: F401
                    Proof, Radix2Dft, StarkConfig, TraceFormat, TwoAdicFriPcs, VerificationError, check_constraints,
                    default_context, prove, prove_batch, prove_batch_lookup, prove_sharded, prove_stream, verify, verify_pre_aux)
from .stark import MultiProof, MultiTableOpening, prove_multi, verify_multi  # noqa: F401
from .stark import MultiBusProof, MultiBusTableOpening, prove_multi_bus, verify_multi_bus  # noqa: F401
from .air import logup_build_multi, logup_multiplicities_bus  # noqa: F401
from .stark import MultiKey, MultiKeyProof, MultiKeyTableOpening, prove_multi_key, verify_multi_key  # noqa: F401
from .air import BusReport, BusShare, bus_check  # noqa: F401
from .stark import check_multi  # noqa: F401
from .derive import DeriveBuilder, derive_check, derive_rows_host  # noqa: F401
from .iterate import IterateBuilder, iterate_check, iterate_rows_host  # noqa: F401
from .scan import ScanSpec, carry_last, running_product, running_sum, scan_rows_host  # noqa: F401
from .collect import CollectSpec, collect_check, collect_rows_host  # noqa: F401
from .stark import collect_rows  # noqa: F401
from .join import JoinSpec, join_check, join_rows_host  # noqa: F401
from .expand import ExpandSpec, expand_check, expand_rows_host  # noqa: F401
from .stark import expand_rows  # noqa: F401
from .group import GroupSpec, group_check, group_rows_host  # noqa: F401
from .stark import group_rows  # noqa: F401
