"""chainpartitioners.jl_amd -- MI355X-native engine for the contiguous sparse-matrix
partitioning hot path of ChainPartitioners.jl (partition_stripe / pack_stripe with the
Dynamic*, BisectCost and Convex methods over the Work / Connectivity / HyperedgeCut /
Block cost oracles).  Host side mirrors the reference's dispatch API; the compute runs in
hand-written HIP kernels behind the C ABI of include/chainpart.h (csrc/).
"""
from .types import *          # noqa: F401,F403
from .types import to_map, to_domain, to_domain_permutation, to_map_permutation   # noqa: F401
from .models import (PowerWorkModel, ConvexWorkModel, ConcaveWorkModel,   # noqa: F401
                     AffineWorkModel, AffinePrimaryConnectivityModel, AffineSecondaryConnectivityModel, AffineConnectivityModel, AffineHyperedgeCutModel,      # noqa: F401
                     AffineSymmetricConnectivityModel, AffineMonotonizedSymmetricConnectivityModel, AffineSymmetricEdgeCutModel,
                     AffinePrimaryEdgeCutModel, AffineSecondaryEdgeCutModel, AffineEnvelopeModel,
                     ColumnBlockComponentCostModel, BlockComponentCostModel, VertexCount, FeasibleCost,
                     ConstrainedCost, EquiSplitter, EquiChunker, StrictChunker, OverlapChunker, DynamicTotalSplitter,
                     DynamicBottleneckSplitter, DynamicTotalChunker, DynamicBottleneckChunker,
                     ReferenceTotalSplitter, ReferenceBottleneckSplitter, ReferenceTotalChunker,
                     BisectCostBottleneckSplitter, FlipBisectCostBottleneckSplitter,
                     BisectIndexBottleneckSplitter, FlipBisectIndexBottleneckSplitter,
                     LazyBisectCostBottleneckSplitter, LazyFlipBisectCostBottleneckSplitter, DisjointPartitioner, AlternatingPartitioner,
                     AlternatingNetPartitioner, SymmetricPartitioner, AlternatingPacker, SymmetricPacker,
                     ConvexTotalChunker, ConvexTotalSplitter, ConcaveTotalChunker, ConcaveTotalSplitter,
                     IdentityPermuter, CuthillMcKeePermuter, PermutingPartitioner,
                     MagneticPartitioner, GreedyBottleneckPartitioner)
from . import _lib  # noqa: F401
from . import draws  # noqa: F401
from .api import (adjointpattern, permute_stripe, permute_plaid, permute, quotientpattern, partition_plaid, pack_plaid, partition_stripe, partition_stripe_batch, pack_stripe, pack_stripe_batch, pack_stripe_tables, oracle_stripe, bound_stripe, total_value,   # noqa: F401
                  bottleneck_value, netcount, selfnetcount, dominancecount, dianetcount, selfpincount, rowenvelope, EnvelopeMatrix, set_default_backend,
                  get_backend, CPError, Step, Same, Next, Prev, Jump)
