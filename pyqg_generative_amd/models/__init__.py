from .parameterization import Parameterization
from .cgan_regression import CGANRegression
from .cvae_regression import CVAERegression
from .mean_var_model import MeanVarModel
from .ols_model import OLSModel
from .ann_model import ANNModel
from .laplace import Laplace
from .physical_parameterizations import (BackscatterBiharmonic, PhysicalParameterization, BackscatterEddy, BackscatterJet,
                                         ZannaBolton, ReynoldsStress, HybridSymbolic, ADM)

__all__ = ['Parameterization', 'CGANRegression', 'CVAERegression', 'MeanVarModel', 'OLSModel', 'ANNModel', 'Laplace',
           'BackscatterBiharmonic', 'PhysicalParameterization', 'BackscatterEddy', 'BackscatterJet', 'ZannaBolton',
           'ReynoldsStress', 'HybridSymbolic', 'ADM']
