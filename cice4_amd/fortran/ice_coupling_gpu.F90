!=======================================================================
! coupling_prep on the GPU for a caller of the reference's driver.
!
! A module of its own name, next to ice_radiation_gpu.  It offers
!   coupling_prep_gpu    what coupling_prep does from `if (oceanmixed_ice) call ocean_mixed_layer (dt)` to the closing
!                        ice_HaloUpdate of scale_factor (drivers/cice4/CICE_RunMod.F90:640-760) as ONE cice_coupling_prep
!                        (include/cice4_amd.h) on the module arrays of ice_flux, ice_state, ice_grid and ice_shortwave.
! The top of coupling_prep -- the time averages a coupled run with a frequency keeps (:611-634) -- stays the driver's.
! A reference compiled -DAusCOM skips scale_fluxes (drivers/access-om/CICE_RunMod.F90:927-959): so does this module
! when it is compiled with that flag.  atmbndy = 'constant' is refused by the library (CICE_EUNSUPPORTED): in that branch
! ocean_mixed_layer multiplies by local arrays it never sets.
! cice_thermo_init and cice_coupling_init are made on the first call, which is after the namelist.
!=======================================================================
      module ice_coupling_gpu

      use ice_kinds_mod
      use ice_domain_size, only: ncat, nilyr, nslyr, max_ntrcr
      use ice_constants
      use iso_c_binding
      use cice4_amd_c

      implicit none
      save
      private
      public :: coupling_prep_gpu

      logical, private :: cpl_ready = .false., batch_ready = .false.
      integer (c_int), allocatable, target, private :: tmask_i4(:,:,:)
      real (c_double), allocatable, target, private :: cnt(:,:,:,:)

      contains

!=======================================================================
      subroutine cpl_ensure
      use ice_state, only: nt_Tsfc, nt_iage
      use ice_age, only: tr_iage
      use ice_therm_vertical, only: heat_capacity, calc_Tsfc, conduct, ustar_min
      use ice_ocean, only: oceanmixed_ice
      use ice_atmo, only: atmbndy
      use ice_blocks, only: nx_block, ny_block
      use ice_domain, only: nblocks
      type (cice_thermo_config) :: tcfg
      type (cice_coupling_config) :: cfg
      real (kind=dbl_kind) :: sal(nilyr+1), tml(nilyr+1)
      if (.not. cpl_ready) then
         call cice_gpu_ensure()
         call cice_gpu_check(cice_check_sizes(cice_gpu_ctx, ncat, nilyr, nslyr, max_ntrcr), 'ice_coupling_gpu')
         tcfg%heat_capacity = merge(1, 0, heat_capacity)
         tcfg%calc_Tsfc = merge(1, 0, calc_Tsfc)
         tcfg%conduct = merge(0, 1, trim(conduct) == 'MU71')
         tcfg%ustar_min = ustar_min
         tcfg%tr_iage = merge(1, 0, tr_iage)
         tcfg%nt_Tsfc = nt_Tsfc
         tcfg%nt_iage = nt_iage
         call cice_gpu_check(cice_thermo_init(cice_gpu_ctx, tcfg, sal, tml), 'cice_thermo_init')
#ifdef AusCOM
         cfg%scale_fluxes = 0
#else
         cfg%scale_fluxes = 1
#endif
         cfg%oceanmixed_ice = merge(1, 0, oceanmixed_ice)
         cfg%atmbndy = merge(1, 0, trim(atmbndy) == 'constant')
         cfg%albocn = albocn
         call cice_gpu_check(cice_coupling_init(cice_gpu_ctx, cfg), 'cice_coupling_init')
         cpl_ready = .true.
      endif
      if (.not. batch_ready) then
         call cice_gpu_check(cice_thermo_batch_alloc(cice_gpu_ctx, nx_block, ny_block, nblocks), 'ice_coupling_gpu')
         batch_ready = .true.
      endif
      end subroutine cpl_ensure

!=======================================================================
! state_resident: aicen is what cice_step_ridge (step_ridge_gpu) left on the device in this step
! alb_resident:   the per-category albedos are what step_radiation_gpu left on the device in this step
! bound:          the library updates the ghost cells of scale_factor (default .true., as the reference does)
      subroutine coupling_prep_gpu (dt, state_resident, alb_resident, bound)
      use ice_blocks, only: nx_block, ny_block
      use ice_domain, only: nblocks
      use ice_calendar, only: nstreams
      use ice_grid, only: tmask
      use ice_state, only: aice, aicen
      use ice_flux
      use ice_shortwave, only: alvdrn, alidrn, alvdfn, alidfn, albicen, albsnon, albpndn
      real (kind=dbl_kind), intent(in) :: dt
      logical (kind=log_kind), intent(in), optional :: state_resident, alb_resident, bound
      type (cice_coupling_fields) :: f

      call cpl_ensure
      f%ncat = ncat
      f%state_resident = 0
      f%alb_resident = 0
      f%bound = 1
      if (present(state_resident)) f%state_resident = merge(1, 0, state_resident)
      if (present(alb_resident)) f%alb_resident = merge(1, 0, alb_resident)
      if (present(bound)) f%bound = merge(1, 0, bound)
      f%nstreams = nstreams
      if (.not. allocated(tmask_i4)) allocate (tmask_i4(nx_block,ny_block,nblocks))
      tmask_i4 = merge(1, 0, tmask(:,:,1:nblocks))
      f%tmask = c_loc(tmask_i4)
      f%alvdrn = addr_r8(alvdrn); f%alidrn = addr_r8(alidrn); f%alvdfn = addr_r8(alvdfn); f%alidfn = addr_r8(alidfn)
      f%albicen = addr_r8(albicen); f%albsnon = addr_r8(albsnon); f%albpndn = addr_r8(albpndn)
      f%aicen = addr_r8(aicen)
      f%coszen = addr_r8(coszen); f%aice = addr_r8(aice); f%Tf = addr_r8(Tf); f%Tair = addr_r8(Tair); f%Qa = addr_r8(Qa)
      f%swvdr = addr_r8(swvdr); f%swvdf = addr_r8(swvdf); f%swidr = addr_r8(swidr); f%swidf = addr_r8(swidf)
      f%strairxT = addr_r8(strairxT); f%strairyT = addr_r8(strairyT); f%fsens = addr_r8(fsens); f%flat = addr_r8(flat)
      f%fswabs = addr_r8(fswabs); f%flwout = addr_r8(flwout); f%evap = addr_r8(evap)
      f%Tref = addr_r8(Tref); f%Qref = addr_r8(Qref)
      f%fresh = addr_r8(fresh); f%fsalt = addr_r8(fsalt); f%fhocn = addr_r8(fhocn); f%fswthru = addr_r8(fswthru)
      f%alvdr = addr_r8(alvdr); f%alidr = addr_r8(alidr); f%alvdf = addr_r8(alvdf); f%alidf = addr_r8(alidf)
      f%albice = addr_r8(albice); f%albsno = addr_r8(albsno); f%albpnd = addr_r8(albpnd)
      f%alvdf_gbm = addr_r8(alvdf_gbm); f%alidf_gbm = addr_r8(alidf_gbm)
      f%alvdr_gbm = addr_r8(alvdr_gbm); f%alidr_gbm = addr_r8(alidr_gbm)
      f%fresh_gbm = addr_r8(fresh_gbm); f%fsalt_gbm = addr_r8(fsalt_gbm)
      f%fhocn_gbm = addr_r8(fhocn_gbm); f%fswthru_gbm = addr_r8(fswthru_gbm)
      f%scale_factor = addr_r8(scale_factor)
      ! albcnt is (nx_block,ny_block,max_blocks,max_nstrm): the library's (nx,ny,nblocks,nstreams) goes through a copy
      f%albcnt = c_null_ptr
      if (nstreams > 0) then
         if (.not. allocated(cnt)) allocate (cnt(nx_block,ny_block,nblocks,nstreams))
         cnt(:,:,:,:) = albcnt(:,:,1:nblocks,1:nstreams)
         f%albcnt = c_loc(cnt)
      endif
      f%potT = addr_r8(potT); f%uatm = addr_r8(uatm); f%vatm = addr_r8(vatm); f%wind = addr_r8(wind)
      f%zlvl = addr_r8(zlvl); f%rhoa = addr_r8(rhoa); f%flw = addr_r8(flw); f%hmix = addr_r8(hmix)
      f%sst = addr_r8(sst); f%qdp = addr_r8(qdp)
      f%frzmlt = addr_r8(frzmlt); f%flwout_ocn = addr_r8(flwout_ocn); f%fsens_ocn = addr_r8(fsens_ocn)
      f%flat_ocn = addr_r8(flat_ocn); f%evap_ocn = addr_r8(evap_ocn)
      f%strairx_ocn = addr_r8(strairx_ocn); f%strairy_ocn = addr_r8(strairy_ocn)
      f%Tref_ocn = addr_r8(Tref_ocn); f%Qref_ocn = addr_r8(Qref_ocn)
      f%alvdr_ocn = addr_r8(alvdr_ocn); f%alidr_ocn = addr_r8(alidr_ocn)
      f%alvdf_ocn = addr_r8(alvdf_ocn); f%alidf_ocn = addr_r8(alidf_ocn)
      f%delt = c_null_ptr; f%delq = c_null_ptr; f%shcoef = c_null_ptr; f%lhcoef = c_null_ptr   ! locals of the reference
      call cice_gpu_check(cice_coupling_prep(cice_gpu_ctx, dt, f), 'coupling_prep_gpu')
      if (nstreams > 0) albcnt(:,:,1:nblocks,1:nstreams) = cnt(:,:,:,:)
      end subroutine coupling_prep_gpu

      end module ice_coupling_gpu
