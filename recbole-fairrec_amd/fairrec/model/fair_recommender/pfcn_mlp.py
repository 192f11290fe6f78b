"""PFCN_MLP: PFCN on an MLP scorer over cat(user, item) (reference: recbole/model/fair_recommender/pfcn_mlp.py).
Tables are named `user_embedding` / `item_embedding`, the scorer `mlp_layer` (registered, trained by optimizer_filter)."""
from ..layers import MLPLayers, dyn_neg_pair_mlp_select, dynamic_neg_scorer_of, full_sort_pair_mlp, full_sort_scorer_of
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

    DYN_NEG_DECLINES = ('_predict_score', '_item_tower', '_user_tower', 'predict', 'forward')

    def dyn_neg_select(self, interaction, cand, num, M):
        """Dynamic negative sampling with `dynamic_neg_scorer: split`: the pick of fr_dyn_neg_mlp_select over this scorer (see
        NFCF.dyn_neg_select).  A filtered model keeps raising the base class's NotImplementedError; `pairs`, a subclass with one
        of DYN_NEG_DECLINES of its own and whatever fairrec/model/layers.py: dyn_neg_pair_mlp_select declines answer None."""
        fused = super().dyn_neg_select(interaction, cand, num, M)      # (raises for a filtered model; None: the scorer is an MLP)
        if fused is not None:
            return fused
        return dyn_neg_pair_mlp_select(self, self.mlp_layer, self.dynamic_neg_scorer, self._utab, self._itab, PFCN_MLP,
                                       PFCN_MLP.DYN_NEG_DECLINES, interaction, cand, num, M)

    def full_sort_pair_mlp(self, interaction, sst_list=None, users_per_batch=None):
        """The pieces of predict() on every item for fr_pair_mlp_scores (`full_sort_scorer: split`), or None: the dense path
        then serves the call.  The users go through the filters as in PFCNBase.full_sort_factors (fast_path.filtered_users).
        No method of a subclass makes it decline."""
        return full_sort_pair_mlp(self, self.mlp_layer, self.full_sort_scorer, self._utab, self._itab, PFCN_MLP, (), interaction,
                                  sst_list, users_per_batch)
