"""PFCN_MLP: PFCN on an MLP scorer over cat(user, item) (reference: recbole/model/fair_recommender/pfcn_mlp.py).
Tables are named `user_embedding` / `item_embedding`, the scorer `mlp_layer` (registered, trained by optimizer_filter)."""
import torch

from ..layers import (MLPLayers, dyn_neg_pair_mlp_pieces, dynamic_neg_scorer_of, full_sort_pair_mlp_pieces,
                      full_sort_scorer_of)
from .pfcn_base import PFCNBase


class PFCN_MLP(PFCNBase):
    biased = False
    user_table_attr = "user_embedding"
    item_table_attr = "item_embedding"

    def _build_base_layers(self, config):
        self.full_sort_scorer = full_sort_scorer_of(config)
        self.dynamic_neg_scorer = dynamic_neg_scorer_of(config)
        self.dropout = config['dropout']
        self.mlp_hidden_size_list = config['mlp_hidden_size_list']
        self.mlp_layer = MLPLayers([self.embedding_size * 2] + list(self.mlp_hidden_size_list) + [1], dropout=self.dropout)

    def _base_dense_modules(self):
        return {"mlp_layer": self.mlp_layer}

    def _score(self, user_embed, item_embed):          # pfcn_mlp.py:185-186, [B, 1]; BPR then averages over B
        return self.mlp_layer(user_embed, item_embed).view(-1)

    def _predict_score(self, ue, ie):
        return self.mlp_layer(ue, ie)

    def dyn_neg_select(self, interaction, cand, num, M):
        """Dynamic negative sampling with `dynamic_neg_scorer: split`: the pick of fr_dyn_neg_mlp_select over this scorer (see
        NFCF.dyn_neg_select).  A filtered model keeps raising the base class's NotImplementedError; `pairs`, a scorer or engine
        the kernel does not serve, a model in training mode with dropout and subclasses with towers of their own answer None."""
        fused = super().dyn_neg_select(interaction, cand, num, M)      # (raises for a filtered model; None: the scorer is an MLP)
        cls, mlp = type(self), self.mlp_layer
        if (fused is not None or self.dynamic_neg_scorer != 'split' or self.shard is not None
                or cls._predict_score is not PFCN_MLP._predict_score or cls._item_tower is not PFCNBase._item_tower
                or cls._user_tower is not PFCNBase._user_tower or cls.predict is not PFCNBase.predict
                or cls.forward is not PFCNBase.forward or (mlp.training and float(mlp.dropout) > 0.0)):
            return fused
        from ...functional import dyn_neg_mlp_select
        eng = self.hip_engine()
        pieces = dyn_neg_pair_mlp_pieces(self.dynamic_neg_scorer, mlp, eng,
                                         lambda: eng.lookup(self._utab, interaction[self.USER_ID]))
        if pieces is None:
            return None
        with torch.no_grad():
            return dyn_neg_mlp_select(pieces, eng._tables[self._itab], eng._hyper(self._itab), cand, num, M, eng.err_flag)

    def full_sort_pair_mlp(self, interaction, sst_list=None, users_per_batch=None):
        """The pieces of predict() on every item for fr_pair_mlp_scores (`full_sort_scorer: split`), or None: the dense path
        then serves the call.  The users go through the filters as in PFCNBase.full_sort_factors: `users_per_batch` at a time
        under batch statistics (the users of one predict() batch of the full-sort evaluation), in any grouping under
        `filter_eval_statistics: running`."""
        if self.shard is not None:
            return None
        eng = self.hip_engine()

        def user_rows():
            ue = eng.lookup(self._utab, interaction[self.USER_ID])
            if self.filter_mode != 'none' and ue.shape[0]:
                per = int(users_per_batch) if users_per_batch else ue.shape[0]
                ue = torch.cat([self._filter(ue[lo:lo + per], sst_list) for lo in range(0, ue.shape[0], per)])
            return ue

        return full_sort_pair_mlp_pieces(self.full_sort_scorer, self.mlp_layer, eng, user_rows, self._itab, self.n_items)
