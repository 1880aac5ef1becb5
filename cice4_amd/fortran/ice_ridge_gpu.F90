!=======================================================================
! ridge_ice on the GPU for a caller of the reference's ice_mechred.
!
! A module of its own name that offers ridge_ice with the reference's interface (source/ice_mechred.F90:133-146) and
! forwards to the block-wise entry cice_ridge_ice of the GPU library (include/cice4_amd.h) through cice4_amd_c.
! It is NOT a drop-in ice_mechred: that module also owns ice_strength and the namelist's ridging parameters, which stay
! where they are -- a caller writes `use ice_ridge_gpu, only: ridge_ice` next to its `use ice_mechred` of the rest.
! cice_itd_init and cice_ridge_init are made on the first call, which is after init_itd and the namelist.
! krdg_redist = 0 is refused by the library (CICE_EUNSUPPORTED; cice4_amd/csrc/ridge.h says why).
! The library addresses trcrn as (nx_block,ny_block,max_ntrcr,ncat); the callers hand in the section
! trcrn(:,:,1:ntrcr,:,iblk), which is copied into an array of that shape and back.
!
! step_ridge_gpu is the one-call form: everything step_dynamics does behind transport_remap (ridge_ice on every block,
! cleanup_itd, bound_state, aggregate, the tendencies; source/ice_step_mod.F90:586-745) as ONE cice_step_ridge on the
! module arrays of ice_state, ice_flux and ice_grid.  It is what a driver needs that keeps the state on the device from
! the transport into ridging (cice_ridge_chain; CICE4_AMD_CHAIN_RIDGE of ice_transport_driver): the seven state arrays
! it names are the ones transport_remap names.  Its first call makes the init calls and allocates the batch, so the
! hand-over starts with the second step.
!=======================================================================
      module ice_ridge_gpu

      use ice_kinds_mod
      use ice_domain_size, only: ncat, nilyr, nslyr, ntilyr, ntslyr, max_ntrcr
      use ice_constants
      use ice_fileunits, only: nu_diag
      use iso_c_binding
      use cice4_amd_c

      implicit none
      save
      private
      public :: ridge_ice, step_ridge_gpu

      logical, private :: ridge_ready = .false., batch_ready = .false.
      integer (c_int), allocatable, target, private :: tmask_i4(:,:,:)

      contains

!=======================================================================
      subroutine ridge_ensure
      use ice_state, only: ntrcr, trcr_depend, nt_Tsfc, nt_iage, nt_alvl, nt_vlvl
      use ice_age, only: tr_iage
      use ice_mechred, only: tr_lvl, krdg_partic, krdg_redist, mu_rdg
      use ice_flux, only: update_ocn_f
      use ice_itd, only: hin_max, hi_min
      type (cice_itd_config) :: cfg
      if (ridge_ready) return
      cfg%ntrcr = ntrcr
      cfg%trcr_depend(:) = 0
      cfg%trcr_depend(1:ntrcr) = trcr_depend(1:ntrcr)
      cfg%nt_Tsfc = nt_Tsfc
      cfg%nt_iage = merge(nt_iage, 0, tr_iage)
      cfg%nt_alvl = merge(nt_alvl, 0, tr_lvl)
      cfg%nt_vlvl = merge(nt_vlvl, 0, tr_lvl)
      cfg%tr_iage = merge(1, 0, tr_iage)
      cfg%tr_lvl = merge(1, 0, tr_lvl)
      cfg%update_ocn_f = merge(1, 0, update_ocn_f)
      cfg%hin_max(1:ncat+1) = hin_max(0:ncat)
      cfg%hi_min = hi_min
      call cice_gpu_ensure()
      call cice_gpu_check(cice_check_sizes(cice_gpu_ctx, ncat, nilyr, nslyr, max_ntrcr), 'ice_ridge_gpu')
      call cice_gpu_check(cice_itd_init(cice_gpu_ctx, cfg), 'cice_itd_init')
      call cice_gpu_check(cice_ridge_init(cice_gpu_ctx, krdg_partic, krdg_redist, mu_rdg), 'cice_ridge_init')
      ridge_ready = .true.
      end subroutine ridge_ensure

!=======================================================================
      subroutine ridge_ice (nx_block,    ny_block,   &
                            dt,          ntrcr,      &
                            icells,                  &
                            indxi,       indxj,      &
                            rdg_conv,    rdg_shear,  &
                            aicen,       trcrn,      &
                            vicen,       vsnon,      &
                            eicen,       esnon,      &
                            aice0,                   &
                            trcr_depend, l_stop,     &
                            istop,       jstop,      &
                            dardg1dt,    dardg2dt,   &
                            dvirdgdt,    opening,    &
                            fresh,       fhocn)
      use ice_itd, only: hin_max
      integer (kind=int_kind), intent(in) :: nx_block, ny_block, icells, ntrcr
      integer (kind=int_kind), dimension (nx_block*ny_block), intent(in) :: indxi, indxj
      real (kind=dbl_kind), intent(in) :: dt
      real (kind=dbl_kind), dimension (nx_block,ny_block), intent(in) :: rdg_conv, rdg_shear
      real (kind=dbl_kind), dimension (nx_block,ny_block,ncat), intent(inout) :: aicen, vicen, vsnon
      real (kind=dbl_kind), dimension (nx_block,ny_block,ntrcr,ncat), intent(inout) :: trcrn
      real (kind=dbl_kind), dimension (nx_block,ny_block,ntilyr), intent(inout) :: eicen
      real (kind=dbl_kind), dimension (nx_block,ny_block,ntslyr), intent(inout) :: esnon
      real (kind=dbl_kind), dimension (nx_block,ny_block), intent(inout) :: aice0
      integer (kind=int_kind), dimension (ntrcr), intent(in) :: trcr_depend
      logical (kind=log_kind), intent(out) :: l_stop
      integer (kind=int_kind), intent(out) :: istop, jstop
      real (kind=dbl_kind), dimension (nx_block,ny_block), intent(inout), optional :: &
         dardg1dt, dardg2dt, dvirdgdt, opening, fresh, fhocn
      real (kind=dbl_kind), allocatable :: tr(:,:,:,:)
      integer (c_int), target :: niter
      integer (c_int) :: ls
      type (c_ptr) :: p(6)

      call ridge_ensure
      hin_max(ncat) = 1.0e+8_dbl_kind    ! the reference's side effect (ridge_prep, ice_mechred.F90:695)
      p(:) = c_null_ptr
      if (present(dardg1dt)) p(1) = addr_r8(dardg1dt)
      if (present(dardg2dt)) p(2) = addr_r8(dardg2dt)
      if (present(dvirdgdt)) p(3) = addr_r8(dvirdgdt)
      if (present(opening))  p(4) = addr_r8(opening)
      if (present(fresh))    p(5) = addr_r8(fresh)
      if (present(fhocn))    p(6) = addr_r8(fhocn)
      allocate (tr(nx_block,ny_block,max_ntrcr,ncat))
      tr = c0
      tr(:,:,1:ntrcr,:) = trcrn
      niter = 0
      call cice_gpu_check(cice_ridge_ice(cice_gpu_ctx, nx_block, ny_block, dt, ntrcr, icells, indxi, indxj, rdg_conv, &
         rdg_shear, aicen, tr, vicen, vsnon, eicen, esnon, aice0, trcr_depend, ls, istop, jstop, p(1), p(2), p(3), &
         p(4), p(5), p(6), c_loc(niter)), 'ridge_ice')
      trcrn = tr(:,:,1:ntrcr,:)
      deallocate (tr)
      l_stop = (ls /= 0)
      if (niter > 1) write(nu_diag,*) 'Repeat ridging (GPU), niter =', niter - 1
      if (l_stop) write(nu_diag,*) 'Ridging error (GPU) at i, j =', istop, jstop, ' after niter =', niter
      end subroutine ridge_ice

!=======================================================================
! stage (0 without a stop): 1 ridge_ice, 2 cleanup_itd; bstop the local block, (istop, jstop) the cell in it -- the
! caller prints them and aborts as step_dynamics does (ice_step_mod.F90:640-649, 683-692)
      subroutine step_ridge_gpu (dt, l_stop, istop, jstop, bstop, stage)
      use ice_blocks, only: nx_block, ny_block
      use ice_domain, only: nblocks
      use ice_grid, only: tmask
      use ice_state, only: aicen, trcrn, vicen, vsnon, eicen, esnon, aice0, aice, vice, vsno, eice, esno, trcr
      use ice_flux, only: rdg_conv, rdg_shear, dardg1dt, dardg2dt, dvirdgdt, opening, fresh, fsalt, fhocn, &
                          daidtd, dvidtd
      use ice_itd, only: hin_max
      real (kind=dbl_kind), intent(in) :: dt
      logical (kind=log_kind), intent(out) :: l_stop
      integer (kind=int_kind), intent(out) :: istop, jstop, bstop, stage
      type (cice_ridge_fields) :: f
      integer (c_int) :: ls

      call ridge_ensure
      if (.not. batch_ready) then
         call cice_gpu_check(cice_thermo_batch_alloc(cice_gpu_ctx, nx_block, ny_block, nblocks), 'step_ridge_gpu')
         allocate (tmask_i4(nx_block,ny_block,nblocks))
         batch_ready = .true.
      endif
      hin_max(ncat) = 1.0e+8_dbl_kind    ! the reference's side effect (ridge_prep, ice_mechred.F90:695)
      tmask_i4 = merge(1, 0, tmask(:,:,1:nblocks))
      f%ncat = ncat
      f%bound = 1
      f%aicen = addr_r8(aicen); f%trcrn = addr_r8(trcrn); f%vicen = addr_r8(vicen); f%vsnon = addr_r8(vsnon)
      f%eicen = addr_r8(eicen); f%esnon = addr_r8(esnon)
      f%tmask = c_loc(tmask_i4)
      f%rdg_conv = addr_r8(rdg_conv); f%rdg_shear = addr_r8(rdg_shear)
      f%aice0 = addr_r8(aice0)
      f%dardg1dt = addr_r8(dardg1dt); f%dardg2dt = addr_r8(dardg2dt); f%dvirdgdt = addr_r8(dvirdgdt)
      f%opening = addr_r8(opening)
      f%aice = addr_r8(aice); f%vice = addr_r8(vice); f%vsno = addr_r8(vsno); f%eice = addr_r8(eice)
      f%esno = addr_r8(esno); f%trcr = addr_r8(trcr)
      f%fresh = addr_r8(fresh); f%fsalt = addr_r8(fsalt); f%fhocn = addr_r8(fhocn)
      f%daidtd = addr_r8(daidtd); f%dvidtd = addr_r8(dvidtd)
      call cice_gpu_check(cice_step_ridge(cice_gpu_ctx, dt, f, ls, istop, jstop, bstop, stage), 'step_ridge_gpu')
      l_stop = (ls /= 0)
      if (l_stop) write(nu_diag,*) 'step_ridge_gpu: stop in stage', stage, ' block', bstop, ' at i, j =', istop, jstop
      end subroutine step_ridge_gpu

      end module ice_ridge_gpu
