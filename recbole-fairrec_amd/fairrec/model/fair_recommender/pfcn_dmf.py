"""PFCN_DMF: PFCN on a two-tower base model with cosine scoring (reference: recbole/model/fair_recommender/pfcn_dmf.py):
`user_mlp` / `item_mlp` towers ([D]*(num_layers+1), mlp_activation, init 'norm') before the filters, scores =
cosine_similarity * 10 in training, sigmoid(cosine) in predict; filters and discriminators use `dis_activation`.

`full_sort_scorer: towers` (default `pairs`: `predict` on every pair) ranks by the dot product of the tower outputs
normalised once per user and once per item -- `full_sort_factors` -- on the fused score-and-select kernels."""
import torch

from ...functional import RowDot
from ..fast_path import config_choice, filtered_users, flushed, single_device_engine
from ..layers import MLPLayers
from .pfcn_base import PFCNBase

COSINE_EPS = 1e-8               # nn.CosineSimilarity's default, as `_cosine` restates it
ITEM_TOWER_ROWS = 1 << 16       # `towers`: the item tower runs over the catalogue this many rows at a time
FUSED_MAX_DIM = 256             # the widest rows the fused ranking kernels (and fr_rows_l2_normalize) take


def dmf_full_sort_scorer_of(config) -> str:
    """The config key `full_sort_scorer` of PFCN_DMF: `pairs` (default: `predict` on every (user, item) pair, the reference)
    or `towers` (each tower once per row, unit rows, the cosine as the fused ranking kernels' dot product)."""
    return config_choice(config, 'full_sort_scorer', ('pairs', 'towers'), 'pairs', of=' of PFCN_DMF')


class PFCN_DMF(PFCNBase):
    biased = False

    def _build_base_layers(self, config):
        self.full_sort_scorer = dmf_full_sort_scorer_of(config)
        self.num_layers = config['num_layers']
        self.mlp_dropout = config['mlp_dropout']
        self.mlp_activation = config['mlp_activation']
        self.dis_activation = config['dis_activation']
        D = self.embedding_size
        mk = lambda: MLPLayers(layers=[D] + [D for _ in range(self.num_layers)], dropout=self.mlp_dropout,
                               activation=self.mlp_activation, init_method='norm')
        self.user_mlp, self.item_mlp = mk(), mk()

    def _base_dense_modules(self):
        return {"user_mlp": self.user_mlp, "item_mlp": self.item_mlp}

    def _filter_activation(self):
        return self.dis_activation

    def _dis_activation(self):
        return self.dis_activation

    def _user_tower(self, rows):
        return self.user_mlp(rows)

    def _item_tower(self, rows):
        return self.item_mlp(rows)

    @staticmethod
    def _cosine(a, b):
        """nn.CosineSimilarity(dim=1, eps=1e-8): a.b / (max(|a|, eps) * max(|b|, eps)); the three row dots are HIP
        launches, the [B]-sized combination is elementwise glue."""
        # clamp before the square root: max(|a|, eps) with a zero (not NaN) gradient for an all-zero row (dead ReLU tower)
        na = torch.sqrt(RowDot.apply(a, a).clamp_min(1e-16))
        nb = torch.sqrt(RowDot.apply(b, b).clamp_min(1e-16))
        return RowDot.apply(a, b) / (na * nb)

    def _score(self, user_embed, item_embed):          # pfcn_dmf.py:193-194
        return self._cosine(user_embed, item_embed) * 10

    def _predict_score(self, ue, ie):
        return self._cosine(ue, ie)

    def full_sort_factors(self, interaction, sst_list=None, users_per_batch=None):
        """`full_sort_scorer: towers`: predict() on every item as the pieces of fr_recommend_topk -- X = the users' filtered
        tower outputs, W = the item tower over the whole (flushed) item table, both with unit rows (fr_rows_l2_normalize, eps =
        1e-8), and the sigmoid as the kernel's epilogue: sigmoid(x^ . w^) = sigmoid(cos(x, w)).  The users go through the
        filters `users_per_batch` at a time, as in PFCNBase.full_sort_factors and for its reason (the filters' BatchNorm
        layers take the statistics of the batch they are given; under `filter_eval_statistics: running` any grouping gives the
        same bits).  The item tower runs over the catalogue once per call, ITEM_TOWER_ROWS rows at a time; nothing is kept
        between calls.  The score differs from predict()'s by the rounding of x^ . w^ against x . w / (|x| |w|).
        None -- the dense path then serves the call -- with `pairs`, on the row-sharded and replicated engines, for rows wider
        than 256, and for a model in training mode whose towers drop out."""
        from ...functional import rows_l2_normalize
        if (self.full_sort_scorer != 'towers' or self.embedding_size > FUSED_MAX_DIM
                or (self.training and float(self.mlp_dropout) > 0.0)):
            return None
        eng = single_device_engine(self)
        if eng is None:
            return None
        user = interaction[self.USER_ID]
        with torch.no_grad():
            if user.numel() == 0:       # an empty request: empty factors on the user side
                ue = torch.empty((0, self.embedding_size), dtype=torch.float32, device=eng.device)
            else:
                ue = filtered_users(self, self._user_tower(eng.lookup(self._utab, user)), sst_list, users_per_batch)
                ue = rows_l2_normalize(ue, eps=COSINE_EPS, out=ue)
            rows = flushed(eng._tables[self._itab], eng._hyper(self._itab))
            W = torch.empty((rows.shape[0], self.embedding_size), dtype=torch.float32, device=rows.device)
            for lo in range(0, rows.shape[0], ITEM_TOWER_ROWS):
                rows_l2_normalize(self._item_tower(rows[lo:lo + ITEM_TOWER_ROWS]), eps=COSINE_EPS, out=W[lo:lo + ITEM_TOWER_ROWS])
            return {'X': ue, 'W': W, 'epilogue': 2}
